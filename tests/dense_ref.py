"""fp64 torch-functional restatement of `MobileNet('nnconv5' / 'nnconv3')` (reference models.py:52-59, 246-270, 420-460: the DENSE NNConv decoder)
built from the product module's own tensors, the layer-local element-wise checks of the dense convolution layers (FD_OP_CONV on fd_conv_gemm), a
narrow hand-made plan driven through the C ABI, and the loader of the golden cases of tools/make_golden_dense.py.  TEST INFRASTRUCTURE ONLY: shared by
the CPU tier (tests/test_dense.py, emulator library) and the GPU tier (tests/test_gpu_dense.py, product library)."""
import ctypes
import functools
import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import harness
from deconv_ref import ABS_FLOOR, REF, UNIT_ROUNDOFF, _triples, reference_modules, spread_err  # noqa: F401  (re-exported to the test files)
from oracle import inputs
from shuffle_ref import _excess, _fold64

capi = harness.capi

# (batch, height, width): 32x32 -- conv1 runs on a 1x1 map (every neighbour is outside the map, M = 2), conv2 on the x2 of a 1x1 map, two images;
# 96x160 -- the maps are 3x5, 6x10, ... (odd, non-square): every M tile is ragged
SHAPES = ((2, 32, 32), (1, 96, 160))
DECODERS = ("nnconv5", "nnconv3")
N_LAYERS = 33                   # 27 encoder units + conv1..conv5 (one dense unit each) + conv6
CONV_AT = [27, 28, 29, 30, 31]


def up(t):
    return F.interpolate(t, scale_factor=2, mode="nearest")


def restate(model, x):
    """-> (output [B,1,H,W], [output of every Conv-BN-act unit in forward order]) in fp64: the reference's forward, nearest x2 after conv1..conv5."""
    outs = []
    t = x.double()
    dec = [getattr(model.decoder, "conv%d" % j) for j in range(1, 7)]
    with torch.no_grad():
        for blk in list(model.mobilenet) + dec:
            for conv, bn, act in _triples(blk):
                t = F.conv2d(t, conv.weight.detach().double(), None, conv.stride, conv.padding, conv.dilation, conv.groups)
                t = F.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
                t = t.clamp(0, 6) if isinstance(act, nn.ReLU6) else t.clamp(min=0)
                outs.append(t)
            if any(blk is d for d in dec[:5]):
                t = up(t)
    return t, outs


@functools.lru_cache(maxsize=None)
def case(decoder, shape):
    """(module, x, fp64 output, fp64 unit outputs) of one small case: computed once, shared by the tests, never modified."""
    b, h, w = shape
    models = inputs.product_models()
    torch.manual_seed(301 + h)
    m = harness.randomize_bn(models.MobileNet(decoder, (h, w), pretrained=False), 302 + h).eval()
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(303 + h))
    y, outs = restate(m, x)
    return m, x, y, outs


@functools.lru_cache(maxsize=None)
def executed(kind, decoder, shape, dtype):
    """A KEEP_ACTIVATIONS plan of the case in `dtype`, run once: (plan, output).  Shared by the tests; only read afterwards."""
    m, x, _, _ = case(decoder, shape)
    device = torch.device("cpu" if kind == "emu" else "cuda")
    plan = harness.CPlan(kind, m, x.to(device), dtype=dtype)
    return plan, plan.forward(x.to(device)).cpu().numpy()


def conv_indices(plan):
    return [i for i, l in enumerate(plan.layers) if l.desc.op == capi.FD_OP_CONV]


def check_whole_network(kind, decoder, shape):
    """Test 1: fp32 plan against the restatement -- every kept unit output and the final output within 1e-3 (harness.rel_err, the project's
    tolerance); 33 layers, the implicit GEMM at 27..31, the existing head with upsample at 32."""
    _, _, y_ref, outs = case(decoder, shape)
    plan, y = executed(kind, decoder, shape, torch.float32)
    info = plan.info()
    errs = [harness.rel_err(plan.tap(i).numpy(), outs[i].numpy()) for i in range(len(outs) - 1)] + [harness.rel_err(y, y_ref.numpy())]
    print("%s %s %s: worst unit error %.3g, output error %.3g" % (kind, decoder, shape, max(errs), errs[-1]))
    assert len(outs) == len(info) == N_LAYERS
    assert conv_indices(plan) == CONV_AT and [i for i, s in enumerate(info) if s.startswith("conv_igemm<k%s" % decoder[6])] == CONV_AT, info
    assert [plan.layers[i].desc.upsample for i in CONV_AT] == [0, 1, 1, 1, 1]
    assert info[32].startswith("head_pw1 up=1"), info[32]
    bad = [(i, e, info[i]) for i, e in enumerate(errs) if not e < 1e-3]
    assert not bad, bad


def _folded(conv, bn):
    s, t = _fold64(bn)
    return s, t, conv.weight.detach().double()


def conv_local_excess(a, y, conv, bn, upsample, dtype, name):
    """Layer-local, element-wise check of one dense convolution layer.  a = the layer's stored input (exact in fp64; upsampled here where the layer
    carries `upsample`), (s, t) = the BatchNorm fold in fp64, r = relu(s conv(a, w) + t), A = |s| conv(|a|, |w|) + |t|, n = k^2 cin:
        hard bound, every element:   |y - r| <= ((n + 8) 2^-24 + u_w) A + u |r| + f
    the any-order worst case of an fp32 dot product of n terms whose folded weights carry one extra rounding (u_w = u = 0 / 2^-11 / 2^-8, the
    rounding of a folded 16-bit weight; u |r|: the stored output; f = 2^-25 for fp16).
        sharp bound, fp32 only:      max |y - r| / (2^-24 A)  <  16 max(rho_ref, 1)
    with rho_ref the same ratio of torch's own fp32 conv2d on the same a and the same folded fp32 weights: the fold's extra rounding, another
    accumulation order and split K each perturb by the order of the reference's own error; a wrong tile or a dropped K block is orders of magnitude off.
    -> (worst |y - r| / hard bound, elements over it, stats, rho_engine or None, rho_ref or None)"""
    k = conv.kernel_size[0]
    a = a.double()
    if upsample:
        a = up(a)
    y = y.double()
    s, t, w = _folded(conv, bn)
    sv, tv = s.view(1, -1, 1, 1), t.view(1, -1, 1, 1)
    r = (F.conv2d(a, w, None, 1, k // 2) * sv + tv).clamp(min=0)
    A = F.conv2d(a.abs(), w.abs(), None, 1, k // 2) * sv.abs() + tv.abs()
    n = k * k * conv.in_channels
    u = UNIT_ROUNDOFF[dtype]
    bound = ((n + 8) * 2.0 ** -24 + u) * A + u * r.abs() + ABS_FLOOR[dtype]
    worst, n_over, st = _excess(y, r, bound, name)
    rho = rho_ref = None
    if dtype == torch.float32:
        wf = (w * s.view(-1, 1, 1, 1)).float()
        y32 = (F.conv2d(a.float(), wf, t.float(), 1, k // 2)).clamp(min=0).double()
        unit = (2.0 ** -24 * A).clamp(min=1e-300)
        rho, rho_ref = float(((y - r).abs() / unit).max()), float(((y32 - r).abs() / unit).max())
    return worst, n_over, st, rho, rho_ref


def plan_conv_excess(plan, i):
    l = plan.layers[i]
    return conv_local_excess(plan.tap(l.desc.src), plan.tap(i), l.conv, l.bn, l.desc.upsample, plan.dtype, l.name)


def assert_local(res, what):
    for worst, n_over, st, rho, rho_ref in res:
        print("%s %s: max |y - r| / hard bound = %.3g, %d elements over, max abs err %.3g%s" % (what, st["layer"], worst, n_over, st["max_abs_err"],
              "" if rho is None else "; rho_engine = %.3g, rho_ref = %.3g (limit %.3g)" % (rho, rho_ref, 16 * max(rho_ref, 1.0))))
    bad = [(worst, n_over, st) for worst, n_over, st, _, _ in res if n_over or not worst <= 1.0]
    assert not bad, bad
    loose = [(st["layer"], rho, rho_ref) for _, _, st, rho, rho_ref in res if rho is not None and not rho < 16 * max(rho_ref, 1.0)]
    assert not loose, loose


def check_layer_local(kind, decoder, shape, dtype):
    """Test 2: every dense convolution layer of a plan in `dtype`, element-wise on the engine's own stored input."""
    plan, _ = executed(kind, decoder, shape, dtype)
    idx = conv_indices(plan)
    assert idx == CONV_AT
    assert_local([plan_conv_excess(plan, i) for i in idx], "%s %s %s %s" % (kind, decoder, shape, dtype))


# ---- the narrow hand-made plan: STEM 3->32, CONV 32->24 k5, CONV 24->40 k3 on up2, PW 40->1 head, on 2 x 32 x 32 ------------------------------
# a cin (24) and a cout (24, 40) that are multiples of no tile, both k, both input compositions; a few milliseconds per forward
NARROW_SHAPE = (2, 32, 32)


def _unit(conv, seed):
    bn = nn.BatchNorm2d(conv.out_channels)
    g = torch.Generator().manual_seed(seed)
    conv.weight.data.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (conv.weight[0].numel())) ** 0.5)
    bn.weight.data.copy_(0.5 + torch.rand(bn.weight.shape, generator=g))
    bn.bias.data.copy_(0.3 * torch.randn(bn.bias.shape, generator=g))
    bn.running_mean.copy_(0.2 * torch.randn(bn.running_mean.shape, generator=g))
    bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=g))
    return conv, bn.eval()


def sparsify(conv):
    """Every (cout) filter keeps exactly one non-zero entry, at input channel (7 co + 3) mod cin and tap co mod k^2: every tap of the layer is used,
    all border taps included, and an output is ONE product plus the bias."""
    cout, cin, k, _ = conv.weight.shape
    w = torch.zeros_like(conv.weight.data)
    for co in range(cout):
        tap = co % (k * k)
        w[co, (7 * co + 3) % cin, tap // k, tap % k] = 1.0 + 0.25 * ((co * 5) % 7)
    conv.weight.data.copy_(w)


@functools.lru_cache(maxsize=None)
def narrow_units(sparse=False):
    """[(name, conv, bn, act, src, upsample)] of the narrow plan; parameters random (sparse: the two CONV layers one tap per filter)."""
    from fastdepth_hip.plan import Layer
    specs = [("stem", nn.Conv2d(3, 32, 3, 2, 1, bias=False), capi.FD_ACT_RELU6, -1, 0), ("conv_a", nn.Conv2d(32, 24, 5, 1, 2, bias=False), capi.FD_ACT_RELU, 0, 0),
             ("conv_b", nn.Conv2d(24, 40, 3, 1, 1, bias=False), capi.FD_ACT_RELU, 1, 1), ("head", nn.Conv2d(40, 1, 1, 1, 0, bias=False), capi.FD_ACT_RELU, 2, 0)]
    layers = []
    with torch.no_grad():
        for q, (name, conv, act, src, ups) in enumerate(specs):
            conv, bn = _unit(conv, 500 + q)
            if sparse and name.startswith("conv_"):
                sparsify(conv)
            layers.append(Layer(name, conv, bn, act, src, ups))
    return layers


def narrow_x():
    return torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(77))


def narrow_restate(layers, x):
    """fp64, plain torch.nn.functional: -> [unit outputs]; the last one is the network output."""
    outs = []
    with torch.no_grad():
        for l in layers:
            t = x.double() if l.desc.src < 0 else outs[l.desc.src]
            if l.desc.upsample:
                t = up(t)
            s, tt = _fold64(l.bn)
            t = F.conv2d(t, l.conv.weight.detach().double(), None, l.conv.stride, l.conv.padding) * s.view(1, -1, 1, 1) + tt.view(1, -1, 1, 1)
            outs.append(t.clamp(0, 6) if l.desc.act == capi.FD_ACT_RELU6 else t.clamp(min=0))
    return outs


class RawPlan(harness.CPlan):
    """A plan built through capi.create_plan from a hand-made list of plan.Layer records instead of a module tree: its own constructor (create or
    import, bind, pack), harness.CPlan's forward / tap / info / export / close."""

    def __init__(self, kind, layers, x, keep=True, dtype=torch.float32, bundle=None):
        self.lib = L = harness.get_lib(kind)
        self.kind, self.model, self.dev, self.dtype, self.layers = kind, None, x.device, dtype, layers
        n = len(layers)
        descs = (capi.LayerDesc * n)(*[l.desc for l in layers])
        self.h = ctypes.c_void_p()
        b, _, hh, ww = x.shape
        if bundle is None:
            capi.check(L, capi.create_plan(L, False, descs, n, b, hh, ww, capi.DTYPE_OF[dtype], capi.FD_PLAN_KEEP_ACTIVATIONS if keep else 0, ctypes.byref(self.h)), "fd_plan_create")
        else:
            capi.check(L, L.fd_plan_import(bundle, len(bundle), b, ctypes.byref(self.h)), "fd_plan_import")
        self.nbytes = L.fd_plan_workspace_bytes(self.h)
        self.fill, self.io, self.pa = None, None, None
        self.ws = torch.empty(self.nbytes + 256, dtype=torch.uint8, device=self.dev)
        self.base = (self.ws.data_ptr() + 255) // 256 * 256
        capi.check(L, L.fd_plan_bind_workspace(self.h, self.base, self.nbytes), "fd_plan_bind_workspace")
        self.stream = torch.cuda.current_stream().cuda_stream if x.is_cuda else None
        if bundle is not None:
            capi.check(L, L.fd_plan_import_weights(self.h, bundle, len(bundle), self.stream), "fd_plan_import_weights")
            return
        params = (capi.LayerParams * n)()
        self._keepalive = []
        for q, l in zip(params, layers):
            for name, t in (("conv_weight", l.conv.weight), ("bn_weight", l.bn.weight), ("bn_bias", l.bn.bias), ("bn_mean", l.bn.running_mean), ("bn_var", l.bn.running_var)):
                t = t.detach().to(self.dev, torch.float32).contiguous()
                self._keepalive.append(t)
                setattr(q, name, t.data_ptr())
        capi.check(L, L.fd_plan_pack_weights(self.h, params, n, layers[0].bn.eps, self.stream), "fd_plan_pack_weights")

    def forward_timed(self, x):
        """fd_forward_timed: -> (y, [ms per layer])"""
        x = x.contiguous()
        y = torch.full((x.shape[0], 1, x.shape[2], x.shape[3]), float("nan"), dtype=torch.float32, device=self.dev)
        ms = (ctypes.c_float * len(self.layers))()
        capi.check(self.lib, self.lib.fd_forward_timed(self.h, x.data_ptr(), y.data_ptr(), self.stream, ms, len(self.layers)), "fd_forward_timed")
        if x.is_cuda:
            torch.cuda.synchronize()
        return y, list(ms)


@functools.lru_cache(maxsize=None)
def narrow_executed(kind, dtype, sparse=False):
    layers = narrow_units(sparse)
    x = narrow_x().to(torch.device("cpu" if kind == "emu" else "cuda"))
    plan = RawPlan(kind, layers, x, dtype=dtype)
    return plan, plan.forward(x).cpu()


def check_narrow(kind, dtype):
    """The narrow plan: the output within 1e-3 of the fp64 restatement (fp32), and both CONV layers element-wise (hard bound; sharp bound in fp32)."""
    layers = narrow_units(False)
    plan, y = narrow_executed(kind, dtype)
    outs = narrow_restate(layers, narrow_x())
    if dtype == torch.float32:
        errs = [harness.rel_err(plan.tap(i).numpy(), outs[i].numpy()) for i in range(3)] + [harness.rel_err(y.numpy(), outs[3].numpy())]
        print("%s narrow plan: unit errors %s" % (kind, ["%.3g" % e for e in errs]))
        assert all(e < 1e-3 for e in errs), errs
    assert float(outs[3].max()) > 0 and all(float((outs[i] > 0).double().mean()) > 0.05 for i in (1, 2))
    assert [s.startswith("conv_igemm<k") for s in plan.info()] == [False, True, True, False], plan.info()
    assert_local([plan_conv_excess(plan, i) for i in (1, 2)], "%s narrow %s" % (kind, dtype))


def one_tap_excess(a, y, conv, bn, upsample, name, dtype=torch.float32):
    """Test 3: with one non-zero weight per filter an output is one product plus the bias, so for every element
        |y - r| <= 8 2^-24 (|s w a| + |t|) + u_w |s w a| + u |r| + f
    -- one wrong tap or K tile among k^2 cin shows.  u_w |s w a|: the one rounding of the folded weight to a 16-bit storage type (the term test 2
    grants per product; u_w = u = 0 / 2^-11 / 2^-8), u |r|: the stored output, f = 2^-25 for fp16."""
    k = conv.kernel_size[0]
    a = a.double()
    if upsample:
        a = up(a)
    s, t, w = _folded(conv, bn)
    sv, tv = s.view(1, -1, 1, 1), t.view(1, -1, 1, 1)
    r = (F.conv2d(a, w, None, 1, k // 2) * sv + tv).clamp(min=0)
    P = F.conv2d(a.abs(), w.abs(), None, 1, k // 2) * sv.abs()                  # (one term per output: |s w a|)
    u = UNIT_ROUNDOFF[dtype]
    return _excess(y.double(), r, 8 * 2.0 ** -24 * (P + tv.abs()) + u * P + u * r.abs() + ABS_FLOOR[dtype], name)


def check_one_tap(kind, dtype=torch.float32):
    layers = narrow_units(True)
    plan, _ = narrow_executed(kind, dtype, True)
    for i in (1, 2):
        l = layers[i]
        kk = l.conv.kernel_size[0] ** 2
        taps = {int(j) for j in torch.nonzero(l.conv.weight.detach().abs().sum((0, 1)).flatten()).flatten()}
        # (conv_a has 24 filters for 25 taps: all but the last corner tap (4, 4), which the full-width layers -- 512 ... 32 filters -- cover; conv_b all 9)
        assert int((l.conv.weight != 0).sum()) == l.conv.out_channels and len(taps) == min(kk, l.conv.out_channels)
        worst, n_over, st = one_tap_excess(plan.tap(l.desc.src), plan.tap(i), l.conv, l.bn, l.desc.upsample, l.name, dtype)
        print("%s one tap %s %s: max |y - r| / bound = %.3g, %d elements over" % (kind, dtype, l.name, worst, n_over))
        assert n_over == 0 and worst <= 1.0, (worst, n_over, st)
        assert float((plan.tap(i) > 0).float().mean()) > 0.05


def check_one_tap_conv1(kind, dtype):
    """decoder.conv1 (1024 -> 512, k 5) of the full-width model at 32 x 32 alone, one non-zero weight per filter (16-bit: 16 K tiles per tap): its map
    is 1 x 1, so every tap but the centre reads the zero line and the outputs of 24 of every 25 filters are the bias alone."""
    import copy
    m, x, _, _ = case("nnconv5", SHAPES[0])
    m = copy.deepcopy(m)
    with torch.no_grad():
        sparsify(m.decoder.conv1[0])
    x = x.to(torch.device("cpu" if kind == "emu" else "cuda"))
    plan = harness.CPlan(kind, m, x, dtype=dtype)
    plan.forward(x)
    l = plan.layers[27]
    worst, n_over, st = one_tap_excess(plan.tap(26), plan.tap(27), l.conv, l.bn, 0, l.name, dtype)
    live = float((plan.tap(27)[:, 12::25] > plan.tap(27)[:, 12::25].min()).float().mean())       # the centre-tap filters see the input
    plan.close()
    print("%s full-width conv1 %s, one tap per filter: max |y - r| / bound = %.3g, %d elements over" % (kind, dtype, worst, n_over))
    assert n_over == 0 and worst <= 1.0, (worst, n_over, st)
    assert live > 0.0


# the 128 x 128 tile (cout >= 128, M >= 1024) and its split-K form, element-wise: decoder.conv3 (256 -> 128 on 28 x 28) of the full-width model at
# (2, 224, 224) has M = 1568 rows in 13 tiles, so its K tiles are split; only that layer is checked (its fp64 reference is 2.6 G multiply-adds)
BIG_SHAPE = (2, 224, 224)


def check_big_tile(kind, decoder, dtype):
    b, h, w = BIG_SHAPE
    models = inputs.product_models()
    torch.manual_seed(311)
    m = harness.randomize_bn(models.MobileNet(decoder, (h, w), pretrained=False), 312).eval()
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(313)).to(torch.device("cpu" if kind == "emu" else "cuda"))
    plan = harness.CPlan(kind, m, x, dtype=dtype)
    plan.forward(x)
    info = plan.info()[29]
    res = [plan_conv_excess(plan, 29)]
    plan.close()
    assert "tile 128x128" in info and "fd_conv_reduce" in info and "M=1568 N=128" in info, info
    assert_local(res, "%s %s %s %s" % (kind, decoder, BIG_SHAPE, dtype))


# ---- golden cases (tools/make_golden_dense.py) ----------------------------------------------------------------------------------------------
def golden_meta():
    with open(os.path.join(inputs.GOLD, "dense.json")) as f:
        return json.load(f)


def golden_model(name):
    """seed -> product constructor, verified against the stored key count and the sha of every conv weight.  -> (module, meta)"""
    meta = golden_meta()[name]
    models = inputs.product_models()
    torch.manual_seed(meta["seed"])
    m = models.MobileNet(meta["decoder"], (224, 224), pretrained=False)
    sd = m.state_dict()
    if len(sd) != meta["keys"]:
        raise AssertionError("state_dict has %d keys, the reference has %d" % (len(sd), meta["keys"]))
    for k, h in meta["conv_weight_sha"].items():
        if inputs._sha(sd[k]) != h:
            raise AssertionError("seeded constructor no longer reproduces reference weights: " + k)
    return m, meta


def golden_case(name):
    """Rebuilds a golden case WITHOUT the reference: golden_model + the stored BatchNorm tensors.  -> (module in eval mode, x, reference output, meta)."""
    m, meta = golden_model(name)
    bn = np.load(os.path.join(inputs.GOLD, name + "_bn.npz"))
    m.load_state_dict({k: torch.from_numpy(bn[k]) for k in bn.files}, strict=False)
    m.eval()
    x = inputs.batch_variants(inputs.load_sample()[0], meta["batch"], meta["seed"])
    y = torch.from_numpy(np.load(os.path.join(inputs.GOLD, name + "_out.npy")))
    return m, x, y, meta


def layer_facts(plan, i):
    L = plan.lib
    b, f, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    capi.check(L, L.fd_plan_layer_stats(plan.h, i, ctypes.byref(b), ctypes.byref(f)), "fd_plan_layer_stats")
    capi.check(L, L.fd_plan_layer_traffic(plan.h, i, ctypes.byref(t)), "fd_plan_layer_traffic")
    return b.value, f.value, t.value, L.fd_plan_kernel_symbol(plan.h, i).decode()
