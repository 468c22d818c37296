"""`MobileNet('nnconv5' / 'nnconv3')` (reference models.py:52-59, 246-270: the DENSE NNConv decoder) on the CPU emulation of the library: the
implicit-GEMM dense convolution fd_conv_gemm (FD_OP_CONV) with its split-K reduction, its plan plumbing, the module surface, the deploy bundle and
the refusals.  The restatement, the bounds and the narrow hand-made plan live in tests/dense_ref.py (shared with the GPU tier)."""
import copy
import ctypes
import os

import pytest
import torch

import dense_ref
import harness
from oracle import inputs

capi = harness.capi
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
SMALL = dense_ref.SHAPES[0]


@pytest.mark.parametrize("decoder", dense_ref.DECODERS)
def test_emulated_dense_forward_matches_restatement(decoder):
    """Test 1 at (2, 32, 32).  The (1, 96, 160) shape runs on the GPU tier only (tests/test_gpu_dense.py): one emulated fp32 forward of it took
    144 s (0.2 G multiply-adds in each of its five dense layers, one fiber switch per lane and MFMA), and the tests need six of them."""
    dense_ref.check_whole_network("emu", decoder, SMALL)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("decoder", dense_ref.DECODERS)
def test_emulated_dense_layers_elementwise(decoder, dtype):
    """Test 2 at (2, 32, 32) (the larger shape: GPU tier, as above)."""
    dense_ref.check_layer_local("emu", decoder, SMALL, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_emulated_narrow_plan(dtype):
    dense_ref.check_narrow("emu", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_emulated_one_tap_at_a_time(dtype):
    dense_ref.check_one_tap("emu", dtype)


def test_emulated_one_tap_full_width_conv1_f16():
    """The full-width conv1 layer (16 K tiles per tap in 16 bit) one tap at a time; the three storage types run on the GPU tier, one of the 16-bit
    ones here (an emulated forward of the model takes about 40 s)."""
    dense_ref.check_one_tap_conv1("emu", torch.float16)


def test_dense_module_surface():
    models = inputs.product_models()
    meta = dense_ref.golden_meta()
    for name in ("nnconv5_s14", "nnconv3_s15"):
        m, info = dense_ref.golden_model(name)                  # key count and the sha of every seeded conv weight == the reference's
        k = int(info["decoder"][6])
        sd = m.state_dict()
        assert len(sd) == info["keys"] == meta[name]["keys"] and [n for n, _ in m.named_children()] == ["mobilenet", "decoder"]
        assert isinstance(m.decoder, models.NNConv) and not isinstance(m.decoder, models.BLConv)
        assert sd["decoder.conv1.0.weight"].shape == (512, 1024, k, k) and sd["decoder.conv5.0.weight"].shape == (32, 64, k, k)
        assert sd["decoder.conv6.0.weight"].shape == (1, 32, 1, 1) and "decoder.conv1.1.running_var" in sd and "decoder.conv1.3.weight" not in sd
    from fastdepth_hip.plan import layers_of
    ls = layers_of(m)
    d = [l.desc for l in ls]
    assert len(ls) == 33 and [l.name for l in ls[27:]] == ["decoder.conv%d.0" % j for j in range(1, 7)]
    assert d[0].op == capi.FD_OP_STEM and all(x.op in (capi.FD_OP_DW, capi.FD_OP_PW) for x in d[1:27])
    assert [(x.op, x.ksize, x.stride, x.cin, x.cout) for x in d[27:32]] == [(capi.FD_OP_CONV, 3, 1, c, c // 2) for c in (1024, 512, 256, 128, 64)]
    assert [x.upsample for x in d[27:]] == [0, 1, 1, 1, 1, 1] and (d[32].op, d[32].cin, d[32].cout) == (capi.FD_OP_PW, 32, 1)
    assert all(x.skip == -1 and x.concat == 0 for x in d) and [x.src for x in d] == [-1] + list(range(32))
    assert capi.FD_OP_CONV == 8 and "conv" in models.__all__
    unit = models.conv(8, 16, 5)
    assert [type(q).__name__ for q in unit] == ["Conv2d", "BatchNorm2d", "ReLU"] and unit[0].padding == (2, 2) and unit[0].bias is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.rand(1, 3, 224, 224))


@pytest.mark.skipif(not os.path.isdir(dense_ref.REF), reason="the reference checkout is not present")
@pytest.mark.parametrize("decoder", dense_ref.DECODERS)
def test_seeded_constructor_matches_reference(decoder):
    models = inputs.product_models()
    torch.manual_seed(23); ours = models.MobileNet(decoder, (224, 224), pretrained=False)
    with dense_ref.reference_modules() as ref_models:
        torch.manual_seed(23); ref = ref_models.MobileNet(decoder, (224, 224), pretrained=False)
        assert type(ref) is not models.MobileNet
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


def test_dense_plan_facts():
    """Test 5: conv_b of the narrow plan (24 -> 40, k 3, on the x2 of the stored 2 x 16 x 16 map): 2 k^2 cin cout flops per output pixel; one read of
    the stored input, one write of the output, the weights in the plan's storage type, the fp32 bias.  Symbols as rocprofv3 prints them."""
    for dtype, esz, tn in ((torch.float32, 4, "float"), (torch.float16, 2, "_Float16"), (torch.bfloat16, 2, "fd_bf16")):
        plan, _ = dense_ref.narrow_executed("emu", dtype)
        b, f, t, sym = dense_ref.layer_facts(plan, 2)
        assert f == 2.0 * 9 * 24 * 40 * (2 * 32 * 32)
        assert b == t == 2 * 16 * 16 * 24 * esz + 2 * 32 * 32 * 40 * esz + 9 * 24 * 40 * esz + 40 * 4
        assert sym == "fd_conv_gemm<%s, 2, 2, 1, 1>" % tn
        b, f, t, sym = dense_ref.layer_facts(plan, 1)
        assert f == 2.0 * 25 * 32 * 24 * (2 * 16 * 16) and b == t == 2 * 16 * 16 * (32 + 24) * esz + 25 * 32 * 24 * esz + 24 * 4
        assert sym == "fd_conv_gemm<%s, 4, 1, 1, 1>" % tn
        info = plan.info()
        assert "split-K 3" in info[1] and "fd_conv_reduce" in info[1] and "on up2" in info[2] and "not pre-summed" in info[1], info


def test_dense_bundle_round_trip_is_bit_equal():
    """A bundle exported from the narrow plan (batch 2) and re-imported with batch_override = 3 reproduces a directly created batch-3 plan bit for bit."""
    layers = dense_ref.narrow_units(False)
    x3 = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(78))
    for dtype in (torch.float32, torch.bfloat16):
        src = dense_ref.RawPlan("emu", layers, dense_ref.narrow_x(), keep=False, dtype=dtype)
        buf = src.export()
        src.close()
        direct = dense_ref.RawPlan("emu", layers, x3, keep=False, dtype=dtype)
        y = direct.forward(x3)
        direct.close()
        imported = dense_ref.RawPlan("emu", layers, x3, keep=False, dtype=dtype, bundle=buf)
        assert [s.startswith("conv_igemm<") for s in imported.info()] == [False, True, True, False]
        y2 = imported.forward(x3)
        imported.close()
        assert not torch.isnan(y).any() and (y > 0).any() and torch.equal(y, y2)


def _create(descs, dtype=capi.FD_F32, train=False, hw=32):
    L = harness.get_lib("emu")
    arr = (capi.LayerDesc * len(descs))(*descs)
    hnd = ctypes.c_void_p()
    capi.check(L, capi.create_plan(L, train, arr, len(descs), 2, hw, hw, dtype, 0, ctypes.byref(hnd)), "fd_plan_create")
    (L.fd_train_plan_destroy if train else L.fd_plan_destroy)(hnd)


def test_dense_refusals():
    models = inputs.product_models()
    for name in ("nnconv7", "upconv", "nnconv9", "upproj", "deconv5", "blconv5", "shuffle3"):
        with pytest.raises(NotImplementedError):
            models.MobileNet(name, (224, 224), pretrained=False)
    for cls in (models.BLConv, models.DeConv, models.ShuffleConv):
        with pytest.raises(NotImplementedError):
            cls(5, False)
    with pytest.raises(NotImplementedError):
        models.NNConv(7, False)
    good = [l.desc for l in dense_ref.narrow_units(False)]

    def edited(i, **kw):
        out = [capi.LayerDesc(*[getattr(d, f) for f, _ in capi.LayerDesc._fields_]) for d in good]
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out
    _create(good)                                               # the accepted form, fp32 and 16-bit
    _create(good, capi.FD_F16)
    msg = r"layer 1: dense convolution \(FD_OP_CONV\) needs k in \{3,5\}, stride 1"
    with pytest.raises(capi.FastDepthError, match=msg):
        _create(edited(1, ksize=7))
    with pytest.raises(capi.FastDepthError, match=msg):
        _create(edited(1, stride=2))
    # a skip tensor whose shape MATCHES the upsampled input, so that only the op's own rule refuses it: on 64 x 64, stem -> 32x32x32, pointwise -> 32x32x24
    # (layer 1, the skip), depthwise stride 2 -> 16x16x24, CONV 24 -> 40 on its x2 with skip = 1, head on the x2 of that
    D = capi.LayerDesc
    skipped = [D(capi.FD_OP_STEM, 3, 32, 3, 2, capi.FD_ACT_RELU6, -1, 0, -1, 0), D(capi.FD_OP_PW, 32, 24, 1, 1, capi.FD_ACT_RELU, 0, 0, -1, 0),
               D(capi.FD_OP_DW, 24, 24, 3, 2, capi.FD_ACT_RELU, 1, 0, -1, 0), D(capi.FD_OP_CONV, 24, 40, 3, 1, capi.FD_ACT_RELU, 2, 1, 1, 0),
               D(capi.FD_OP_PW, 40, 1, 1, 1, capi.FD_ACT_RELU, 3, 1, -1, 0)]
    with pytest.raises(capi.FastDepthError, match=r"layer 3: dense convolution \(FD_OP_CONV\).*no skip / concat"):
        _create(skipped, hw=64)
    skipped[3].skip = -1
    _create(skipped, hw=64)                                     # (the same plan without the skip is accepted)
    # concat never reaches the op's rule: the plan's general rule admits it for depthwise consumers only, and names the layer
    with pytest.raises(capi.FastDepthError, match=r"layer 2: concat needs an upsampled depthwise consumer"):
        _create(edited(2, skip=0, concat=1))
    # src = -1: a dense convolution on the network input
    with pytest.raises(capi.FastDepthError, match=r"layer 0: dense convolution \(FD_OP_CONV\)"):
        _create(edited(0, op=capi.FD_OP_CONV, ksize=3, stride=1, cout=32))
    with pytest.raises(capi.FastDepthError, match=msg.replace("layer 1", "layer 2")):
        _create(edited(2, upsample=2))
    def with_pw(cmid):                                          # stem 3 -> 32, pointwise 32 -> cmid, CONV cmid -> 40 on up2, head
        e = edited(1, op=capi.FD_OP_PW, ksize=1, cout=cmid)
        e[2].cin = cmid
        return e
    _create(with_pw(28))                                        # 28 % 4 == 0: accepted by an fp32 plan ...
    with pytest.raises(capi.FastDepthError, match=r"layer 2: dense convolution \(FD_OP_CONV\).*multiples of 8"):
        _create(with_pw(28), capi.FD_BF16)                      # ... and refused in 16 bit
    with pytest.raises(capi.FastDepthError, match=r"layer 2: dense convolution \(FD_OP_CONV\).*multiples of 4"):
        _create(with_pw(22))
    with pytest.raises(capi.FastDepthError, match=r"layer 1: dense convolution \(FD_OP_CONV\).*multiples of 4"):
        _create(edited(1, cout=22) [:2] + edited(2, cin=22)[2:])


def test_train_plans_refuse_dense_units():
    msg = r"layer 1: dense convolution units \(FD_OP_CONV\) run in inference plans only; their train step is not implemented"
    with pytest.raises(capi.FastDepthError, match=msg):
        _create([l.desc for l in dense_ref.narrow_units(False)], train=True)
    m, x, _, _ = dense_ref.case("nnconv3", SMALL)
    msg27 = msg.replace("layer 1", "layer 27")
    with pytest.raises(capi.FastDepthError, match=msg27):
        harness.CTrainPlan("emu", m, x)
    from fastdepth_hip.train import TrainEngine
    eng = TrainEngine(copy.deepcopy(m).train(), _library=harness.get_lib("emu"))
    with pytest.raises(capi.FastDepthError, match=msg27):
        eng.step(x, torch.rand(2, 1, 32, 32))


def test_depthwise_sibling_selection_is_untouched():
    """The depthwise-separable sibling of the same shape: no dense layer in its walk, the stem still the stem."""
    models = inputs.product_models()
    torch.manual_seed(203)
    m = models.MobileNet("nnconv5dw", (32, 32), pretrained=False).eval()
    from fastdepth_hip.plan import layers_of
    d = [l.desc for l in layers_of(m)]
    assert len(d) == 38 and d[0].op == capi.FD_OP_STEM and not any(x.op == capi.FD_OP_CONV for x in d)
