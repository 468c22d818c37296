"""`MobileNet('shuffle5dw' / 'shuffle3dw')` (reference models.py:296-333: the ShuffleConv decoder, depthwise form) on the CPU emulation of the
library: the pixel-shuffle depthwise kernel fd_dws_rows (FD_OP_DWS), the pixel-shuffle tail fd_head_shuffle (FD_OP_PWS), their plan plumbing,
the module surface, the deploy bundle and the refusals.  The restatement and the layer-local bounds live in tests/shuffle_ref.py (shared with
the GPU tier)."""
import ctypes
import os

import pytest
import torch

import harness
import shuffle_ref
from oracle import inputs

REF = shuffle_ref.REF
capi = harness.capi


@pytest.mark.parametrize("shape", shuffle_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", shuffle_ref.DECODERS)
def test_emulated_shuffle_forward_matches_restatement(decoder, shape):
    shuffle_ref.check_whole_network("emu", decoder, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", shuffle_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", shuffle_ref.DECODERS)
def test_emulated_shuffle_layers_elementwise(decoder, shape, dtype):
    shuffle_ref.check_layer_local("emu", decoder, shape, dtype)


def test_shuffle_module_surface():
    models = inputs.product_models()
    m = models.MobileNet("shuffle5dw", (224, 224), pretrained=False)
    sd = m.state_dict()
    bn_keys = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    want = []
    for j in range(1, 5):
        for q in (0, 1):
            want += ["decoder.conv%d.%d.0.weight" % (j, q)] + ["decoder.conv%d.%d.1.%s" % (j, q, s) for s in bn_keys]
    keys = list(sd)
    assert len(keys) == 210 and keys[0] == "mobilenet.0.0.weight" and keys[162:] == want and all(k.startswith("mobilenet.") for k in keys[:162])
    assert sorted({k.split(".")[1] for k in keys[:162]}, key=int) == [str(i) for i in range(14)]
    assert sd["decoder.conv1.0.0.weight"].shape == (256, 1, 5, 5) and sd["decoder.conv4.1.0.weight"].shape == (4, 4, 1, 1)
    assert isinstance(m.decoder, models.ShuffleConv) and not hasattr(m.decoder, "conv5")
    assert models.MobileNet("shuffle3dw", (224, 224), pretrained=False).state_dict()["decoder.conv2.0.0.weight"].shape == (64, 1, 3, 3)
    # He-normal init through weights_init (n = k * k * out_channels, reference models.py:36-40)
    assert abs(float(m.decoder.conv1[0][0].weight.detach().std()) - (2.0 / (25 * 256)) ** 0.5) < 5e-4
    from fastdepth_hip.plan import layers_of
    ls = layers_of(m)
    assert len(ls) == 35
    assert [l.name for l in ls[27:]] == ["decoder.conv%d.%d" % (j, q) for j in range(1, 5) for q in (0, 1)]
    d = [l.desc for l in ls]
    assert [(x.op, x.ksize, x.stride) for x in d[27:35:2]] == [(capi.FD_OP_DWS, 5, 1)] * 4 and [x.cin for x in d[27:35:2]] == [256, 64, 16, 4]
    assert [x.op for x in d[28:35:2]] == [capi.FD_OP_PW] * 3 + [capi.FD_OP_PWS] and [(x.cin, x.cout) for x in d[28:35:2]] == [(256, 256), (64, 64), (16, 16), (4, 4)]
    assert all(x.op in (capi.FD_OP_STEM, capi.FD_OP_DW, capi.FD_OP_PW) for x in d[:27])
    assert all(x.upsample == 0 and x.skip == -1 and x.concat == 0 for x in d) and [x.src for x in d] == [-1] + list(range(34))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.rand(1, 3, 224, 224))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not present")
@pytest.mark.parametrize("decoder", shuffle_ref.DECODERS)
def test_seeded_constructor_and_pickle_match_reference(decoder, tmp_path):
    models = inputs.product_models()
    torch.manual_seed(17); ours = models.MobileNet(decoder, (224, 224), pretrained=False)
    with shuffle_ref.reference_modules() as ref_models:
        torch.manual_seed(17); ref = ref_models.MobileNet(decoder, (224, 224), pretrained=False)
        assert type(ref) is not models.MobileNet
        path = str(tmp_path / "ckpt.pth.tar")
        torch.save({"epoch": 1, "model": ref}, path)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b) and len(a) == 210
    assert all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    loaded = torch.load(path, weights_only=False)["model"]      # unpickles into the product classes: models.MobileNet / models.ShuffleConv
    assert type(loaded) is models.MobileNet and type(loaded.decoder) is models.ShuffleConv
    assert all(torch.equal(v, b[k]) for k, v in loaded.state_dict().items())
    plan = harness.CPlan("emu", loaded.eval(), torch.rand(1, 3, 32, 32), keep=False)
    info = plan.info()
    plan.close()
    assert sum(s.startswith("dws_rows<") for s in info) == 4 and info[-1].startswith("head_shuffle<")


def test_shuffle_bundle_round_trip_is_bit_equal():
    m, x, _, _ = shuffle_ref.case("shuffle5dw", (2, 32, 32))
    x = x[:1].contiguous()                                      # (1, 32, 32): two emulated forwards of one image
    plan = harness.CPlan("emu", m, x, keep=False)
    y = plan.forward(x)
    L = plan.lib
    n = L.fd_plan_export_bytes(plan.h)
    buf = (ctypes.c_ubyte * n)()
    capi.check(L, L.fd_plan_export(plan.h, buf, n, None), "fd_plan_export")
    plan.close()
    h = ctypes.c_void_p()
    capi.check(L, L.fd_plan_import(buf, n, 0, ctypes.byref(h)), "fd_plan_import")
    try:
        info = [L.fd_plan_kernel_info(h, i).decode() for i in range(L.fd_plan_num_kernels(h))]
        assert sum(s.startswith("dws_rows<k5") for s in info) == 4 and info[-1].startswith("head_shuffle<")
        nbytes = L.fd_plan_workspace_bytes(h)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8)
        base = (ws.data_ptr() + 255) // 256 * 256
        capi.check(L, L.fd_plan_bind_workspace(h, base, nbytes), "fd_plan_bind_workspace")
        capi.check(L, L.fd_plan_import_weights(h, buf, n, None), "fd_plan_import_weights")
        y2 = torch.full_like(y, float("nan"))
        capi.check(L, L.fd_forward(h, x.contiguous().data_ptr(), y2.data_ptr(), None), "fd_forward")
    finally:
        L.fd_plan_destroy(h)
    assert not torch.isnan(y).any() and torch.equal(y, y2)


def test_shuffle_plan_statistics():
    """DWS: 2 k^2 flops per output, one read of src and one write (the same element count), taps and bias.  PWS: a pointwise layer (2 cin flops per
    output element) with a 4-byte output and fp32 weights in every plan."""
    m, x, _, _ = shuffle_ref.case("shuffle3dw", (2, 32, 32))
    res = {}
    for dtype in (torch.float32, torch.float16):
        plan = harness.CPlan("emu", m, x, keep=False, dtype=dtype)
        L = plan.lib
        for i in (29, 34):                                      # decoder.conv2.0: 64 channels, source 2x2x256 -> 4x4x64; decoder.conv4.1: 4 -> 4 on 16x16
            b, f, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            capi.check(L, L.fd_plan_layer_stats(plan.h, i, ctypes.byref(b), ctypes.byref(f)), "fd_plan_layer_stats")
            capi.check(L, L.fd_plan_layer_traffic(plan.h, i, ctypes.byref(t)), "fd_plan_layer_traffic")
            res[dtype, i] = (b.value, f.value, t.value, L.fd_plan_kernel_symbol(plan.h, i).decode())
        plan.close()
    for dtype, esz, tn in ((torch.float32, 4, "float"), (torch.float16, 2, "_Float16")):
        b, f, t, sym = res[dtype, 29]
        assert f == 2.0 * 9 * (2 * 4 * 4 * 64)
        assert b == t == (2 * 2 * 2 * 256 + 2 * 4 * 4 * 64) * esz + 9 * 64 * 4 + 2 * 64 * 4
        assert sym == "fd_dws_rows<%s, 3, 1>" % tn
        b, f, t, sym = res[dtype, 34]
        assert f == 2.0 * 4 * (2 * 16 * 16 * 4)
        assert b == t == 2 * 16 * 16 * 4 * esz + 2 * 16 * 16 * 4 * 4 + 4 * 4 * 4 + 2 * 4 * 4
        assert sym == "fd_head_shuffle<%s, 1>" % tn


def _create(descs, b=1, h=32, w=32, dtype=capi.FD_F32):
    L = harness.get_lib("emu")
    arr = (capi.LayerDesc * len(descs))(*descs)
    hnd = ctypes.c_void_p()
    capi.check(L, capi.create_plan(L, False, arr, len(descs), b, h, w, dtype, 0, ctypes.byref(hnd)), "fd_plan_create")
    L.fd_plan_destroy(hnd)


def test_shuffle_refusals():
    models = inputs.product_models()
    for name in ("shuffle5", "shuffle7dw", "deconv5", "deconv7dw", "deconv3"):
        with pytest.raises(NotImplementedError):
            models.MobileNet(name, (224, 224), pretrained=False)
    with pytest.raises(NotImplementedError):
        models.ShuffleConv(5, False)
    from fastdepth_hip.plan import layers_of
    m, _, _, _ = shuffle_ref.case("shuffle3dw", (2, 32, 32))
    good = [l.desc for l in layers_of(m)]

    def edited(i, **kw):
        out = [capi.LayerDesc(*[getattr(d, f) for f, _ in capi.LayerDesc._fields_]) for d in good]
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out
    _create(good)                                               # the accepted form
    with pytest.raises(capi.FastDepthError, match="only valid as the last layer"):
        _create(edited(32, op=capi.FD_OP_PWS, cout=4) + [])     # (conv3.1 16 -> 4 as a tail in the middle)
    with pytest.raises(capi.FastDepthError, match="cout==4"):
        _create(edited(34, cout=8))
    with pytest.raises(capi.FastDepthError, match="producer channels"):
        _create(edited(29, cin=32, cout=32))                    # 4 * 32 != 256
    with pytest.raises(capi.FastDepthError, match="no upsample / skip / concat"):
        _create(edited(29, upsample=1))
    with pytest.raises(capi.FastDepthError, match="no upsample / skip / concat|skip"):
        _create(edited(29, skip=3))
    with pytest.raises(capi.FastDepthError, match="the last layer must produce"):
        _create(good[:34])                                      # (without the tail the last layer is a 4-channel map of half the size)


def test_train_plans_refuse_pixel_shuffle_units():
    m, x, _, _ = shuffle_ref.case("shuffle5dw", (2, 32, 32))
    msg = r"layer 27: pixel-shuffle units \(FD_OP_DWS\) run in inference plans only"
    with pytest.raises(capi.FastDepthError, match=msg):
        harness.CTrainPlan("emu", m, x)
    from fastdepth_hip.train import TrainEngine
    import copy
    eng = TrainEngine(copy.deepcopy(m).train(), _library=harness.get_lib("emu"))
    with pytest.raises(capi.FastDepthError, match=msg):
        eng.step(x, torch.rand(2, 1, 32, 32))
    # the tail alone is refused with its own name
    from fastdepth_hip.plan import layers_of
    descs = [layers_of(m)[0].desc, capi.LayerDesc(capi.FD_OP_PWS, 32, 4, 1, 1, capi.FD_ACT_RELU, 0, 0, -1, 0)]      # stem, then the tail
    L = harness.get_lib("emu")
    arr = (capi.LayerDesc * len(descs))(*descs)
    hnd = ctypes.c_void_p()
    with pytest.raises(capi.FastDepthError, match=r"layer 1: pixel-shuffle units \(FD_OP_PWS\) run in inference plans only"):
        capi.check(L, capi.create_plan(L, True, arr, len(descs), 2, 32, 32, capi.FD_F32, 0, ctypes.byref(hnd)), "fd_train_plan_create")
