"""fp64 torch-functional restatement of `MobileNet('deconv5dw' / 'deconv3dw')` (reference models.py:145-180, 420-460) built from the
product module's own tensors, the layer-local element-wise check of the transposed depthwise layers (FD_OP_DWT, fd_dwt_rows), and the
loader of the golden cases of tools/make_golden_deconv.py.  TEST INFRASTRUCTURE ONLY: shared by the CPU tier (tests/test_deconv.py,
emulator library) and the GPU tier (tests/test_gpu_deconv.py, product library)."""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import harness
from oracle import inputs

# (batch, height, width): 32x32 -- the maps run 1x1 -> 32x32 (every neighbour of the first transposed layer is outside the map) with two
# images; 96x160 -- the first map is 3x5 (odd, non-square), ragged strips of work-items on every map
SHAPES = ((2, 32, 32), (1, 96, 160))
DECODERS = ("deconv5dw", "deconv3dw")
UNIT_ROUNDOFF = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
ABS_FLOOR = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}      # fp16: half the smallest subnormal


REF = "/root/reference"
_SHADOWED = ("models", "metrics", "imagenet", "imagenet.mobilenet")


@contextlib.contextmanager
def reference_modules():
    """The reference's `models` module, importable as `models` while the block runs (its classes pickle under that name); the product's modules
    of the same names are put back afterwards."""
    from oracle.make_golden import import_reference
    saved = {k: sys.modules.pop(k) for k in _SHADOWED if k in sys.modules}
    try:
        ref_models, _ = import_reference()
        yield ref_models
    finally:
        for k in _SHADOWED:
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def _triples(seq):
    flat = []

    def walk(m):
        if isinstance(m, torch.nn.Sequential):
            for c in m:
                walk(c)
        else:
            flat.append(m)
    walk(seq)
    assert len(flat) % 3 == 0
    return [flat[i:i + 3] for i in range(0, len(flat), 3)]


def _conv64(t, conv):
    w = conv.weight.detach().double()
    if isinstance(conv, torch.nn.ConvTranspose2d):
        return F.conv_transpose2d(t, w, None, conv.stride, conv.padding, conv.output_padding, conv.groups, conv.dilation)
    return F.conv2d(t, w, None, conv.stride, conv.padding, conv.dilation, conv.groups)


def restate(model, x):
    """-> (output, [output of every Conv-BN-act unit in forward order]) in fp64."""
    outs = []
    t = x.double()
    blocks = list(model.mobilenet) + [getattr(model.decoder, "convt%d" % j) for j in range(1, 6)] + [model.decoder.convf]
    with torch.no_grad():
        for blk in blocks:
            for conv, bn, act in _triples(blk):
                t = _conv64(t, conv)
                t = F.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
                t = t.clamp(0, 6) if isinstance(act, torch.nn.ReLU6) else t.clamp(min=0)
                outs.append(t)
    return t, outs


@functools.lru_cache(maxsize=None)
def case(decoder, shape):
    """(module, x, fp64 output, fp64 unit outputs) of one small case: computed once, shared by the tests, never modified."""
    b, h, w = shape
    models = inputs.product_models()
    torch.manual_seed(41 + h)
    m = harness.randomize_bn(models.MobileNet(decoder, (h, w), pretrained=False), 42 + h).eval()
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(43 + h))
    y, outs = restate(m, x)
    return m, x, y, outs


def dwt_indices(plan):
    return [i for i, l in enumerate(plan.layers) if l.desc.op == harness.capi.FD_OP_DWT]


def dwt_local_excess(plan, i):
    """Layer-local, element-wise check of transposed depthwise layer i of an executed KEEP_ACTIVATIONS plan.  With a = the engine's own stored
    input (exact in fp64), (s, t) = the BatchNorm fold in fp64, r = relu(s convT(a, w) + t) and A = |s| convT(|a|, |w|) + |t|:
        |y - r| <= 64 * 2^-24 * A  +  u |r|  +  f
    64 * 2^-24: the fp32 fold takes at most ~8 roundings per tap, the accumulation of at most 9 products 9, the bias fold 4 = ~21 half-ulps of the
    absolute-value sum, times a margin of three; u |r|: the one rounding of the stored output (u = 0 / 2^-11 / 2^-8); f = 2^-25 for fp16 (half the
    smallest subnormal).  Returns (largest |y - r| / bound, number of elements over the bound, stats for the message)."""
    l = plan.layers[i]
    conv, bn = l.conv, l.bn
    a = plan.tap(l.desc.src).double()
    y = plan.tap(i).double()
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t = bn.bias.detach().double() - bn.running_mean.double() * s
    w = conv.weight.detach().double()
    args = (None, conv.stride, conv.padding, conv.output_padding, conv.groups, conv.dilation)
    r = (F.conv_transpose2d(a, w, *args) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).clamp(min=0)
    A = F.conv_transpose2d(a.abs(), w.abs(), *args) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
    bound = 64 * 2.0 ** -24 * A + UNIT_ROUNDOFF[plan.dtype] * r.abs() + ABS_FLOOR[plan.dtype]
    assert y.shape == r.shape, (y.shape, r.shape)
    d = (y - r).abs()
    ratio = torch.where(bound > 0, d / bound.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    worst = int(ratio.argmax())
    return float(ratio.max()), int((d > bound).sum()), {"layer": l.name, "shape": tuple(y.shape), "worst_index": np.unravel_index(worst, tuple(y.shape)),
                                                        "y": float(y.flatten()[worst]), "r": float(r.flatten()[worst]), "max_abs_err": float(d.max())}


def spread_err(y, y_ref):
    """max |y - y_ref| / (max y_ref - min y_ref): the calibrated head sits at ~2.8 with a spread of ~0.2, so the max-norm of harness.rel_err would
    hide a wrong decoder."""
    y, y_ref = np.asarray(y, np.float64), np.asarray(y_ref, np.float64)
    return float(np.abs(y - y_ref).max() / (y_ref.max() - y_ref.min()))


def golden_meta():
    with open(os.path.join(inputs.GOLD, "deconv.json")) as f:
        return json.load(f)


def golden_case(name):
    """Rebuilds a golden case of tools/make_golden_deconv.py WITHOUT the reference: seed -> product constructor (bit-identical parameters,
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
    """A KEEP_ACTIVATIONS plan of the case in `dtype`, run once: (plan, output).  Shared by the tests (the emulator takes ~20 s per full-width
    forward); only read afterwards."""
    m, x, _, _ = case(decoder, shape)
    device = torch.device("cpu" if kind == "emu" else "cuda")
    plan = harness.CPlan(kind, m, x.to(device), dtype=dtype)
    return plan, plan.forward(x.to(device)).cpu().numpy()


def check_whole_network(kind, decoder, shape):
    """Case 1: fp32 plan against the restatement -- every kept unit output and the final output within 1e-3 (harness.rel_err, the project's
    tolerance), exactly five dwt_rows layers, none of them fused."""
    _, _, y_ref, outs = case(decoder, shape)
    plan, y = executed(kind, decoder, shape, torch.float32)
    info = plan.info()
    idx = dwt_indices(plan)
    errs = [harness.rel_err(plan.tap(i).numpy(), outs[i].numpy()) for i in range(len(outs) - 1)] + [harness.rel_err(y, y_ref.numpy())]
    print("%s %s %s: worst unit error %.3g, output error %.3g" % (kind, decoder, shape, max(errs), errs[-1]))
    assert len(outs) == len(info) == 38
    assert idx == [27, 29, 31, 33, 35] and [i for i, s in enumerate(info) if s.startswith("dwt_rows<k%s" % decoder[6])] == idx, info
    assert not any("fused" in info[i] for i in idx), [info[i] for i in idx]
    bad = [(i, e, info[i]) for i, e in enumerate(errs) if not e < 1e-3]
    assert not bad, bad


def check_layer_local(kind, decoder, shape, dtype):
    """Case 2: every transposed depthwise layer of a plan in `dtype`, element-wise on the engine's own stored input."""
    plan, _ = executed(kind, decoder, shape, dtype)
    idx = dwt_indices(plan)
    res = [dwt_local_excess(plan, i) for i in idx]
    for worst, n_over, st in res:
        print("%s %s %s %s %s: max |y - r| / bound = %.3g, %d elements over, max abs err %.3g" % (kind, decoder, shape, dtype, st["layer"], worst, n_over, st["max_abs_err"]))
    assert len(idx) == 5
    bad = [(worst, n_over, st) for worst, n_over, st in res if n_over or not worst <= 1.0]
    assert not bad, bad
