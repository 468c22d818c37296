"""fp64 torch-functional restatement of `MobileNet('blconv5dw' / 'blconv3dw')` (reference models.py:272-294, 420-460) built from the product
module's own tensors, the layer-local element-wise checks of the bilinear layers (FD_OP_DWB on fd_dwb_rows, FD_OP_PWB on fd_head_bilinear),
and the loader of the golden cases of tools/make_golden_bilinear.py.  TEST INFRASTRUCTURE ONLY: shared by the CPU tier (tests/test_bilinear.py,
emulator library) and the GPU tier (tests/test_gpu_bilinear.py, product library)."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import harness
from deconv_ref import ABS_FLOOR, REF, UNIT_ROUNDOFF, _triples, reference_modules, spread_err  # noqa: F401  (re-exported to the test files)
from oracle import inputs
from shuffle_ref import _excess, _fold64

# (batch, height, width): 32x32 -- the DWB sources run 1x1 -> 8x8 and the head reads 16x16 (a 1x1 source is all clamping and mostly padding) with
# two images; 96x160 -- the first source is 3x5 (odd, non-square): ragged strips of work-items and band halos on every map
SHAPES = ((2, 32, 32), (1, 96, 160))
DECODERS = ("blconv5dw", "blconv3dw")
# (8 fold roundings + k^2 products + 4 interpolation roundings + 4 bias-fold roundings) half-ulps x 3, rounded up to a power of two:
# k = 3: 75 -> 128, k = 5: 123 -> 128 (shuffle_ref.C_K's derivation with the interpolation added)
C_K = {3: 128, 5: 128}
C_PWB = 256         # the head: 3 x (64 products + 8 fold + 4 interpolation + 4 bias) = 240 half-ulps -> 256
N_LAYERS = 38       # 27 encoder units + conv1..conv5 (two each) + conv6
DWB_AT = [29, 31, 33, 35]       # decoder.conv2.0 .. conv5.0 (27 = decoder.conv1.0 is a plain depthwise layer on the encoder output)
SHARE = (0.05, 0.97)            # admissible share of positive outputs


def up(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)


def last_bn(model):
    return model.decoder.conv6[1]


def _decoder_blocks(model):
    return [getattr(model.decoder, "conv%d" % j) for j in range(1, 7)]


def calibrate_last_bn(model, x):
    """Running statistics of the last BatchNorm (decoder.conv6[1], one channel) := the batch statistics of its own input on x (one pass, that module
    alone in train mode, momentum 1).  With arbitrary statistics the 1-channel output is dead (all zero behind the ReLU) and shows nothing."""
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
            for j, blk in enumerate(_decoder_blocks(model), 1):
                t = blk(t)
                if j <= 5:
                    t = up(t)
    finally:
        bn.momentum = mom
        model.train(was)
    return model


def positive_share(y):
    return float((torch.as_tensor(y) > 0).double().mean())


def restate(model, x):
    """-> (output [B,1,H,W], [output of every Conv-BN-act unit in forward order]) in fp64: the reference's forward, F.interpolate after conv1..conv5."""
    outs = []
    t = x.double()
    dec = _decoder_blocks(model)
    with torch.no_grad():
        for blk in list(model.mobilenet) + dec:
            for conv, bn, act in _triples(blk):
                t = F.conv2d(t, conv.weight.detach().double(), None, conv.stride, conv.padding, conv.dilation, conv.groups)
                t = F.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
                t = t.clamp(0, 6) if isinstance(act, torch.nn.ReLU6) else t.clamp(min=0)
                outs.append(t)
            if any(blk is d for d in dec[:5]):
                t = up(t)
    return t, outs


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
    share = positive_share(y)
    assert SHARE[0] <= share <= SHARE[1], "a dead (or all-positive) output shows nothing of the head's ReLU: share of positive outputs %.3f" % share
    return m, x, y, outs


def dwb_indices(plan):
    return [i for i, l in enumerate(plan.layers) if l.desc.op == harness.capi.FD_OP_DWB]


def dwb_local_excess(plan, i):
    """Layer-local, element-wise check of bilinear depthwise layer i of an executed KEEP_ACTIVATIONS plan.  With a = the engine's own stored input
    (exact in fp64), (s, t) = the BatchNorm fold in fp64, r = relu(s conv2d(up(a), w) + t) and A = |s| conv2d(up(|a|), |w|) + |t| (up has
    non-negative weights, so A bounds any evaluation order, composed taps included):
        |y - r| <= c_k * 2^-24 * A  +  u |r|  +  f,    c_3 = c_5 = 128 (C_K above)
    u |r|: the one rounding of the stored output (u = 0 / 2^-11 / 2^-8); f = 2^-25 for fp16 (half the smallest subnormal)."""
    l = plan.layers[i]
    conv, bn = l.conv, l.bn
    k = conv.kernel_size[0]
    a = plan.tap(l.desc.src).double()
    y = plan.tap(i).double()
    s, t = _fold64(bn)
    w = conv.weight.detach().double()
    args = (None, 1, k // 2, 1, conv.groups)
    r = (F.conv2d(up(a), w, *args) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).clamp(min=0)
    A = F.conv2d(up(a.abs()), w.abs(), *args) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
    bound = C_K[k] * 2.0 ** -24 * A + UNIT_ROUNDOFF[plan.dtype] * r.abs() + ABS_FLOOR[plan.dtype]
    return _excess(y, r, bound, l.name)


def pwb_local_excess(plan, y):
    """The same for the head (the last layer) on the stored conv5.1 output against the final y: r = relu(up(s pw(a) + t)),
    A = up(|s| pw(|a|) + |t|), c = 256, and u = f = 0 in every dtype -- fp32 weights and an fp32 output make the only 16-bit rounding its input,
    which is taken as given."""
    i = len(plan.layers) - 1
    l = plan.layers[i]
    assert l.desc.op == harness.capi.FD_OP_PWB
    a = plan.tap(l.desc.src).double()
    s, t = _fold64(l.bn)
    w = l.conv.weight.detach().double()
    r = up(F.conv2d(a, w) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).clamp(min=0)
    A = up(F.conv2d(a.abs(), w.abs()) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1))
    return _excess(torch.as_tensor(y).double(), r, C_PWB * 2.0 ** -24 * A, l.name)


def golden_meta():
    with open(os.path.join(inputs.GOLD, "bilinear.json")) as f:
        return json.load(f)


def golden_case(name):
    """Rebuilds a golden case of tools/make_golden_bilinear.py WITHOUT the reference: seed -> product constructor (bit-identical parameters,
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
    tolerance); 38 layers, dwb_rows at 29 / 31 / 33 / 35, head_bilinear at 37, none of them fused."""
    _, _, y_ref, outs = case(decoder, shape)
    plan, y = executed(kind, decoder, shape, torch.float32)
    info = plan.info()
    idx = dwb_indices(plan)
    errs = [harness.rel_err(plan.tap(i).numpy(), outs[i].numpy()) for i in range(len(outs) - 1)] + [harness.rel_err(y, y_ref.numpy())]
    print("%s %s %s: worst unit error %.3g, output error %.3g" % (kind, decoder, shape, max(errs), errs[-1]))
    assert len(outs) == len(info) == N_LAYERS
    assert idx == DWB_AT and [i for i, s in enumerate(info) if s.startswith("dwb_rows<k%s" % decoder[6])] == idx, info
    assert info[N_LAYERS - 1].startswith("head_bilinear<"), info[N_LAYERS - 1]
    assert not any("fused" in info[i] for i in idx + [N_LAYERS - 1]), [info[i] for i in idx + [N_LAYERS - 1]]
    bad = [(i, e, info[i]) for i, e in enumerate(errs) if not e < 1e-3]
    assert not bad, bad


def check_layer_local(kind, decoder, shape, dtype):
    """Check 2: every bilinear layer of a plan in `dtype`, element-wise on the engine's own stored input."""
    plan, y = executed(kind, decoder, shape, dtype)
    idx = dwb_indices(plan)
    res = [dwb_local_excess(plan, i) for i in idx] + [pwb_local_excess(plan, y)]
    for worst, n_over, st in res:
        print("%s %s %s %s %s: max |y - r| / bound = %.3g, %d elements over, max abs err %.3g" % (kind, decoder, shape, dtype, st["layer"], worst, n_over, st["max_abs_err"]))
    assert len(idx) == 4
    bad = [(worst, n_over, st) for worst, n_over, st in res if n_over or not worst <= 1.0]
    assert not bad, bad
