"""fp64 torch-functional restatement of `MobileNet('shuffle5dw' / 'shuffle3dw')` (reference models.py:296-333, 420-460) built from the product
module's own tensors, the layer-local element-wise checks of the pixel-shuffle layers (FD_OP_DWS on fd_dws_rows, FD_OP_PWS on fd_head_shuffle),
and the loader of the golden cases of tools/make_golden_shuffle.py.  TEST INFRASTRUCTURE ONLY: shared by the CPU tier (tests/test_shuffle.py,
emulator library) and the GPU tier (tests/test_gpu_shuffle.py, product library)."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import harness
from deconv_ref import ABS_FLOOR, REF, UNIT_ROUNDOFF, _triples, reference_modules, spread_err  # noqa: F401  (re-exported to the test files)
from oracle import inputs

# (batch, height, width): 32x32 -- the source maps run 1x1 -> 16x16 (conv1.0 sees a 2x2 map with nearly every tap outside) with two images;
# 96x160 -- the first source map is 3x5 (odd, non-square): ragged strips of work-items and band halos on every map
SHAPES = ((2, 32, 32), (1, 96, 160))
DECODERS = ("shuffle5dw", "shuffle3dw")
# (8 fold roundings + k^2 products + 4 bias-fold roundings) half-ulps x 3, rounded up to a power of two: k = 3: 63 -> 64, k = 5: 111 -> 128
C_K = {3: 64, 5: 128}
C_PWS = 64          # the pointwise tail: at most 64 products


def last_bn(model):
    return model.decoder.conv4[1][1]


def calibrate_last_bn(model, x):
    """Running statistics of the last BatchNorm := the batch statistics of its own input on x (one pass, that module alone in train mode, momentum
    1).  A 4-channel BatchNorm with arbitrary statistics leaves whole output phases dead, and a dead phase hides a wrong channel -> phase map."""
    bn = last_bn(model)
    was, mom = model.training, bn.momentum
    model.eval()
    bn.train()
    bn.momentum = 1.0
    try:
        with torch.no_grad():
            t = x
            for blk in model.mobilenet:
                t = blk(t)
            for j in range(1, 5):
                t = getattr(model.decoder, "conv%d" % j)(F.pixel_shuffle(t, 2))
    finally:
        bn.momentum = mom
        model.train(was)
    return model


def phase_shares(y):
    """share of positive elements of the four output phases y[:, :, i::2, j::2]"""
    y = torch.as_tensor(y)
    return [float((y[:, :, i::2, j::2] > 0).double().mean()) for i in (0, 1) for j in (0, 1)]


def restate(model, x):
    """-> (output [B,1,H,W], [output of every Conv-BN-act unit in forward order]) in fp64."""
    outs = []
    t = x.double()
    dec = [getattr(model.decoder, "conv%d" % j) for j in range(1, 5)]
    with torch.no_grad():
        for blk in list(model.mobilenet) + dec:
            if any(blk is d for d in dec):
                t = F.pixel_shuffle(t, 2)
            for conv, bn, act in _triples(blk):
                t = F.conv2d(t, conv.weight.detach().double(), None, conv.stride, conv.padding, conv.dilation, conv.groups)
                t = F.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
                t = t.clamp(0, 6) if isinstance(act, torch.nn.ReLU6) else t.clamp(min=0)
                outs.append(t)
        y = F.pixel_shuffle(t, 2)
    return y, outs


@functools.lru_cache(maxsize=None)
def case(decoder, shape):
    """(module, x, fp64 output, fp64 unit outputs) of one small case: computed once, shared by the tests, never modified."""
    b, h, w = shape
    models = inputs.product_models()
    torch.manual_seed(203)
    m = harness.randomize_bn(models.MobileNet(decoder, (h, w), pretrained=False), 204).eval()
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(205))
    calibrate_last_bn(m, x)
    m.eval()
    y, outs = restate(m, x)
    shares = phase_shares(y)
    assert all(0.15 <= s <= 0.85 for s in shares), "a dead output phase would hide a wrong channel -> phase map: %s" % (shares,)
    return m, x, y, outs


def dws_indices(plan):
    return [i for i, l in enumerate(plan.layers) if l.desc.op == harness.capi.FD_OP_DWS]


def _fold64(bn):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.double() * s


def _excess(y, r, bound, name):
    assert y.shape == r.shape, (y.shape, r.shape)
    d = (y - r).abs()
    ratio = torch.where(bound > 0, d / bound.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    worst = int(ratio.argmax())
    return float(ratio.max()), int((d > bound).sum()), {"layer": name, "shape": tuple(y.shape), "worst_index": np.unravel_index(worst, tuple(y.shape)),
                                                        "y": float(y.flatten()[worst]), "r": float(r.flatten()[worst]), "max_abs_err": float(d.max())}


def dws_local_excess(plan, i):
    """Layer-local, element-wise check of pixel-shuffle depthwise layer i of an executed KEEP_ACTIVATIONS plan, in the style of
    deconv_ref.dwt_local_excess.  With a = the engine's own stored input (exact in fp64), (s, t) = the BatchNorm fold in fp64,
    r = relu(s conv2d(pixel_shuffle(a), w) + t) and A = |s| conv2d(pixel_shuffle(|a|), |w|) + |t|:
        |y - r| <= c_k * 2^-24 * A  +  u |r|  +  f,    c_3 = 64, c_5 = 128 (C_K above)
    u |r|: the one rounding of the stored output (u = 0 / 2^-11 / 2^-8); f = 2^-25 for fp16 (half the smallest subnormal)."""
    l = plan.layers[i]
    conv, bn = l.conv, l.bn
    k = conv.kernel_size[0]
    a = plan.tap(l.desc.src).double()
    y = plan.tap(i).double()
    s, t = _fold64(bn)
    w = conv.weight.detach().double()
    args = (None, 1, k // 2, 1, conv.groups)
    r = (F.conv2d(F.pixel_shuffle(a, 2), w, *args) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).clamp(min=0)
    A = F.conv2d(F.pixel_shuffle(a.abs(), 2), w.abs(), *args) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
    bound = C_K[k] * 2.0 ** -24 * A + UNIT_ROUNDOFF[plan.dtype] * r.abs() + ABS_FLOOR[plan.dtype]
    return _excess(y, r, bound, l.name)


def pws_local_excess(plan, y):
    """The same for the pointwise tail (the last layer) on the stored conv4.0 output against the final y: c = 64, and u = f = 0 in every dtype --
    fp32 weights and an fp32 output make the only 16-bit rounding its input, which is taken as given."""
    i = len(plan.layers) - 1
    l = plan.layers[i]
    assert l.desc.op == harness.capi.FD_OP_PWS
    a = plan.tap(l.desc.src).double()
    s, t = _fold64(l.bn)
    w = l.conv.weight.detach().double()
    r = F.pixel_shuffle((F.conv2d(a, w) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).clamp(min=0), 2)
    A = F.pixel_shuffle(F.conv2d(a.abs(), w.abs()) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1), 2)
    return _excess(torch.as_tensor(y).double(), r, C_PWS * 2.0 ** -24 * A, l.name)


def golden_meta():
    with open(os.path.join(inputs.GOLD, "shuffle.json")) as f:
        return json.load(f)


def golden_case(name):
    """Rebuilds a golden case of tools/make_golden_shuffle.py WITHOUT the reference: seed -> product constructor (bit-identical parameters,
    verified against the stored sha of every conv weight) + the stored BatchNorm tensors.  -> (module in eval mode, x, reference output, meta)."""
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
    bn = np.load(os.path.join(inputs.GOLD, name + "_bn.npz"))
    m.load_state_dict({k: torch.from_numpy(bn[k]) for k in bn.files}, strict=False)
    m.eval()
    x = inputs.batch_variants(inputs.load_sample()[0], meta["batch"], meta["seed"])
    y = torch.from_numpy(np.load(os.path.join(inputs.GOLD, name + "_out.npy")))
    return m, x, y, meta


@functools.lru_cache(maxsize=None)
def executed(kind, decoder, shape, dtype):
    """A KEEP_ACTIVATIONS plan of the case in `dtype`, run once: (plan, output).  Shared by the tests; only read afterwards."""
    m, x, _, _ = case(decoder, shape)
    device = torch.device("cpu" if kind == "emu" else "cuda")
    plan = harness.CPlan(kind, m, x.to(device), dtype=dtype)
    return plan, plan.forward(x.to(device)).cpu().numpy()


def check_whole_network(kind, decoder, shape):
    """Check 1: fp32 plan against the restatement -- every kept unit output and the final output within 1e-3 (harness.rel_err, the project's
    tolerance); 35 layers, dws_rows at 27 / 29 / 31 / 33, head_shuffle at 34, none of them fused."""
    _, _, y_ref, outs = case(decoder, shape)
    plan, y = executed(kind, decoder, shape, torch.float32)
    info = plan.info()
    idx = dws_indices(plan)
    errs = [harness.rel_err(plan.tap(i).numpy(), outs[i].numpy()) for i in range(len(outs) - 1)] + [harness.rel_err(y, y_ref.numpy())]
    print("%s %s %s: worst unit error %.3g, output error %.3g" % (kind, decoder, shape, max(errs), errs[-1]))
    assert len(outs) == len(info) == 35
    assert idx == [27, 29, 31, 33] and [i for i, s in enumerate(info) if s.startswith("dws_rows<k%s" % decoder[7])] == idx, info
    assert info[34].startswith("head_shuffle<"), info[34]
    assert not any("fused" in info[i] for i in idx + [34]), [info[i] for i in idx + [34]]
    bad = [(i, e, info[i]) for i, e in enumerate(errs) if not e < 1e-3]
    assert not bad, bad


def check_layer_local(kind, decoder, shape, dtype):
    """Check 2: every pixel-shuffle layer of a plan in `dtype`, element-wise on the engine's own stored input."""
    plan, y = executed(kind, decoder, shape, dtype)
    idx = dws_indices(plan)
    res = [dws_local_excess(plan, i) for i in idx] + [pws_local_excess(plan, y)]
    for worst, n_over, st in res:
        print("%s %s %s %s %s: max |y - r| / bound = %.3g, %d elements over, max abs err %.3g" % (kind, decoder, shape, dtype, st["layer"], worst, n_over, st["max_abs_err"]))
    assert len(idx) == 4
    bad = [(worst, n_over, st) for worst, n_over, st in res if n_over or not worst <= 1.0]
    assert not bad, bad
