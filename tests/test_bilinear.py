"""`MobileNet('blconv5dw' / 'blconv3dw')` (reference models.py:272-294: the BLConv decoder, depthwise form) on the CPU emulation of the
library: the bilinear depthwise kernel fd_dwb_rows (FD_OP_DWB), the bilinear head fd_head_bilinear (FD_OP_PWB), their plan plumbing, the
module surface, the deploy bundle and the refusals.  The restatement and the layer-local bounds live in tests/bilinear_ref.py (shared with
the GPU tier)."""
import ctypes
import os

import pytest
import torch

import bilinear_ref
import harness
from oracle import inputs

REF = bilinear_ref.REF
capi = harness.capi


@pytest.mark.parametrize("shape", bilinear_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", bilinear_ref.DECODERS)
def test_emulated_bilinear_forward_matches_restatement(decoder, shape):
    bilinear_ref.check_whole_network("emu", decoder, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", bilinear_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", bilinear_ref.DECODERS)
def test_emulated_bilinear_layers_elementwise(decoder, shape, dtype):
    bilinear_ref.check_layer_local("emu", decoder, shape, dtype)


def test_bilinear_module_surface():
    models = inputs.product_models()
    m = models.MobileNet("blconv5dw", (224, 224), pretrained=False)
    sib = models.MobileNet("nnconv5dw", (224, 224), pretrained=False)
    sd = m.state_dict()
    assert len(sd) == 228 and list(sd) == list(sib.state_dict()) and all(sd[k].shape == v.shape for k, v in sib.state_dict().items())
    assert isinstance(m.decoder, models.BLConv) and issubclass(models.BLConv, models.NNConv) and not isinstance(sib.decoder, models.BLConv)
    assert models.BLConv.__mro__[:2] == (models.BLConv, models.NNConv) and "BLConv" in models.__all__
    assert sd["decoder.conv2.0.0.weight"].shape == (512, 1, 5, 5) and sd["decoder.conv6.0.weight"].shape == (1, 32, 1, 1)
    assert models.MobileNet("blconv3dw", (224, 224), pretrained=False).state_dict()["decoder.conv2.0.0.weight"].shape == (512, 1, 3, 3)
    from fastdepth_hip.plan import layers_of
    ls = layers_of(m)
    assert len(ls) == 38
    assert [l.name for l in ls[27:]] == ["decoder.conv%d.%d" % (j, q) for j in range(1, 6) for q in (0, 1)] + ["decoder.conv6.0"]
    d = [l.desc for l in ls]
    assert (d[27].op, d[27].ksize, d[27].stride, d[27].cin) == (capi.FD_OP_DW, 5, 1, 1024)                      # conv1.0: the 7x7 encoder output as it is
    assert [(x.op, x.ksize, x.stride) for x in d[29:37:2]] == [(capi.FD_OP_DWB, 5, 1)] * 4 and [(x.cin, x.cout) for x in d[29:37:2]] == [(c, c) for c in (512, 256, 128, 64)]
    assert [x.op for x in d[28:37:2]] == [capi.FD_OP_PW] * 5 and [(x.cin, x.cout) for x in d[28:37:2]] == [(c, c // 2) for c in (1024, 512, 256, 128, 64)]
    assert (d[37].op, d[37].cin, d[37].cout, d[37].ksize) == (capi.FD_OP_PWB, 32, 1, 1)
    assert all(x.op in (capi.FD_OP_STEM, capi.FD_OP_DW, capi.FD_OP_PW) for x in d[:27])
    assert all(x.upsample == 0 and x.skip == -1 and x.concat == 0 for x in d) and [x.src for x in d] == [-1] + list(range(37))
    assert (capi.FD_OP_DWB, capi.FD_OP_PWB) == (6, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.rand(1, 3, 224, 224))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not present")
@pytest.mark.parametrize("decoder", bilinear_ref.DECODERS)
def test_seeded_constructor_and_pickle_match_reference(decoder, tmp_path):
    models = inputs.product_models()
    torch.manual_seed(17); ours = models.MobileNet(decoder, (224, 224), pretrained=False)
    with bilinear_ref.reference_modules() as ref_models:
        torch.manual_seed(17); ref = ref_models.MobileNet(decoder, (224, 224), pretrained=False)
        assert type(ref) is not models.MobileNet
        path = str(tmp_path / "ckpt.pth.tar")
        torch.save({"epoch": 1, "model": ref}, path)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b) and len(a) == 228
    assert all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    loaded = torch.load(path, weights_only=False)["model"]      # unpickles into the product classes: models.MobileNet / models.BLConv
    assert type(loaded) is models.MobileNet and type(loaded.decoder) is models.BLConv
    assert all(torch.equal(v, b[k]) for k, v in loaded.state_dict().items())
    plan = harness.CPlan("emu", loaded.eval(), torch.rand(1, 3, 32, 32), keep=False)
    info = plan.info()
    plan.close()
    assert sum(s.startswith("dwb_rows<") for s in info) == 4 and info[-1].startswith("head_bilinear<")


def test_bilinear_bundle_round_trip_is_bit_equal():
    m, x, _, _ = bilinear_ref.case("blconv5dw", (2, 32, 32))
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
        assert sum(s.startswith("dwb_rows<k5") for s in info) == 4 and info[-1].startswith("head_bilinear<")
        nbytes = L.fd_plan_workspace_bytes(h)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8)
        base = (ws.data_ptr() + 255) // 256 * 256
        capi.check(L, L.fd_plan_bind_workspace(h, base, nbytes), "fd_plan_bind_workspace")
        capi.check(L, L.fd_plan_import_weights(h, buf, n, None), "fd_plan_import_weights")
        y2 = torch.full_like(y, float("nan"))
        capi.check(L, L.fd_forward(h, x.contiguous().data_ptr(), y2.data_ptr(), None), "fd_forward")
    finally:
        L.fd_plan_destroy(h)
    assert not torch.isnan(y).any() and (y > 0).any() and torch.equal(y, y2)


def test_bilinear_plan_statistics():
    """DWB: 2 k^2 flops per output element (the interpolation is not counted), one read of the source map and one write of the four times larger
    output, taps and bias: 5 B h w C esz + (k^2 + 2) C 4 bytes.  Head: 2 cin flops per SOURCE pixel; B h w cin esz + 16 B h w + cin 4 + 8 bytes
    (fp32 weights and a 4-byte output in every plan)."""
    m, x, _, _ = bilinear_ref.case("blconv3dw", (2, 32, 32))
    res = {}
    for dtype in (torch.float32, torch.float16):
        plan = harness.CPlan("emu", m, x, keep=False, dtype=dtype)
        L = plan.lib
        for i in (31, 37):                                      # decoder.conv3.0: 256 channels, source 2x2 -> 4x4; decoder.conv6.0: 32 -> 1 on 16x16 -> 32x32
            b, f, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            capi.check(L, L.fd_plan_layer_stats(plan.h, i, ctypes.byref(b), ctypes.byref(f)), "fd_plan_layer_stats")
            capi.check(L, L.fd_plan_layer_traffic(plan.h, i, ctypes.byref(t)), "fd_plan_layer_traffic")
            res[dtype, i] = (b.value, f.value, t.value, L.fd_plan_kernel_symbol(plan.h, i).decode())
        plan.close()
    for dtype, esz, tn in ((torch.float32, 4, "float"), (torch.float16, 2, "_Float16")):
        b, f, t, sym = res[dtype, 31]
        assert f == 2.0 * 9 * (2 * 4 * 4 * 256)
        assert b == t == 5 * 2 * 2 * 2 * 256 * esz + (9 + 2) * 256 * 4
        assert sym == "fd_dwb_rows<%s, 3, 1>" % tn
        b, f, t, sym = res[dtype, 37]
        assert f == 2.0 * 32 * (2 * 16 * 16)
        assert b == t == 2 * 16 * 16 * 32 * esz + 16 * 2 * 16 * 16 + 32 * 4 + 8
        assert sym == "fd_head_bilinear<%s, 1>" % tn


def _create(descs, b=1, h=32, w=32, dtype=capi.FD_F32):
    L = harness.get_lib("emu")
    arr = (capi.LayerDesc * len(descs))(*descs)
    hnd = ctypes.c_void_p()
    capi.check(L, capi.create_plan(L, False, arr, len(descs), b, h, w, dtype, 0, ctypes.byref(hnd)), "fd_plan_create")
    L.fd_plan_destroy(hnd)


def test_bilinear_refusals():
    models = inputs.product_models()
    for name in ("blconv5", "blconv7dw", "blconv3", "blconv9dw"):
        with pytest.raises(NotImplementedError):
            models.MobileNet(name, (224, 224), pretrained=False)
    with pytest.raises(NotImplementedError):
        models.BLConv(5, False)
    from fastdepth_hip.plan import layers_of
    m, _, _, _ = bilinear_ref.case("blconv3dw", (2, 32, 32))
    good = [l.desc for l in layers_of(m)]

    def edited(i, **kw):
        out = [capi.LayerDesc(*[getattr(d, f) for f, _ in capi.LayerDesc._fields_]) for d in good]
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out
    _create(good)                                               # the accepted form
    with pytest.raises(capi.FastDepthError, match=r"FD_OP_PWB\) is only valid as the last layer"):
        _create(edited(36, op=capi.FD_OP_PWB, cout=1))          # (conv5.1 64 -> 1 as a head in the middle)
    with pytest.raises(capi.FastDepthError, match=r"FD_OP_PWB\).*cout==1"):
        _create(edited(37, cout=4))
    with pytest.raises(capi.FastDepthError, match=r"FD_OP_DWB\).*producer channels"):
        _create(edited(31, cin=128, cout=128))                  # the producer (conv2.1) has 256 channels
    with pytest.raises(capi.FastDepthError, match=r"FD_OP_DWB\).*no upsample / skip / concat"):
        _create(edited(31, upsample=1))
    with pytest.raises(capi.FastDepthError, match=r"FD_OP_DWB\).*no upsample / skip / concat|skip"):
        _create(edited(31, skip=3))
    with pytest.raises(capi.FastDepthError, match="the last layer must produce"):
        _create(good[:37])                                      # (without the head the last layer is a 32-channel map of half the size)
    with pytest.raises(capi.FastDepthError, match="the last layer must produce"):
        _create(good[:36])                                      # (... or the DWB map itself)


def test_train_plans_refuse_bilinear_units():
    m, x, _, _ = bilinear_ref.case("blconv5dw", (2, 32, 32))
    msg = r"layer 29: bilinear-upsampling units \(FD_OP_DWB\) run in inference plans only"
    with pytest.raises(capi.FastDepthError, match=msg):
        harness.CTrainPlan("emu", m, x)
    from fastdepth_hip.train import TrainEngine
    import copy
    eng = TrainEngine(copy.deepcopy(m).train(), _library=harness.get_lib("emu"))
    with pytest.raises(capi.FastDepthError, match=msg):
        eng.step(x, torch.rand(2, 1, 32, 32))
    # the head alone is refused with its own name
    from fastdepth_hip.plan import layers_of
    descs = [layers_of(m)[0].desc, capi.LayerDesc(capi.FD_OP_PWB, 32, 1, 1, 1, capi.FD_ACT_RELU, 0, 0, -1, 0)]      # stem, then the head
    L = harness.get_lib("emu")
    arr = (capi.LayerDesc * len(descs))(*descs)
    hnd = ctypes.c_void_p()
    with pytest.raises(capi.FastDepthError, match=r"layer 1: bilinear-upsampling units \(FD_OP_PWB\) run in inference plans only"):
        capi.check(L, capi.create_plan(L, True, arr, len(descs), 2, 32, 32, capi.FD_F32, 0, ctypes.byref(hnd)), "fd_train_plan_create")


def test_nnconv_sibling_selection_is_untouched():
    """The NNConv sibling of the same shape: neither new kernel appears in its plan, and its head stays the nearest-upsampling fd_head_pw1."""
    models = inputs.product_models()
    torch.manual_seed(203)
    m = models.MobileNet("nnconv5dw", (32, 32), pretrained=False).eval()
    plan = harness.CPlan("emu", m, torch.rand(2, 3, 32, 32), keep=False)
    info = plan.info()
    plan.close()
    assert len(info) == 38 and not any("dwb_rows" in s or "head_bilinear" in s for s in info), info
    from fastdepth_hip.plan import layers_of
    assert not any(l.desc.op in (capi.FD_OP_DWB, capi.FD_OP_PWB) for l in layers_of(m)) and layers_of(m)[-1].desc.upsample == 1
