"""nn.Module tree -> list of fused layers for fd_plan_create.

Shapes are discovered from the instance's sub-modules at call time, never from constructor arguments:
reference checkpoints are whole pickled modules whose __init__ is bypassed on load (main.py:49-57),
and pruned models carry irregular widths.  The walk restates the reference's forward order
(models.py:706-732): conv0..conv13, skip taps after conv1/conv3/conv5, decode_conv1..5 each followed
by nearest x2 and (after 2/3/4) the additive skip, then decode_conv6.  Upsample + add are not layers of
their own: they become `upsample` / `skip` attributes of the layer that consumes the result.  The DeConv decoder of the no-skip sibling
(`decoder.convt1..5`, `decoder.convf`) upsamples nowhere: its depthwise transposed convolutions are layers of their own kind (FD_OP_DWT).
The ShuffleConv decoder (`decoder.conv1..4`) puts a 2x pixel shuffle before each unit and after the last: its depthwise layers read through the
shuffle (FD_OP_DWS) and its last pointwise layer writes the network output through it (FD_OP_PWS).
The BLConv decoder (`decoder.conv1..6`, class attribute `_fd_upsample = "bilinear"`) puts a bilinear x2 after conv1..conv5: the depthwise layers
of conv2..conv5 interpolate their producer's output themselves (FD_OP_DWB), and conv6 is evaluated before the last interpolation (FD_OP_PWB).
The dense NNConv decoder (`MobileNet('nnconv5' / 'nnconv3')`: `decoder.conv1..5` are ONE dense k x k unit each) takes the same walk as its
depthwise-separable sibling: its units become FD_OP_CONV layers, conv2..conv5 and the head carrying `upsample`.
"""
import torch.nn as nn

from . import capi


def _act_of(mod):
    if isinstance(mod, nn.ReLU6):
        return capi.FD_ACT_RELU6
    if isinstance(mod, nn.ReLU):
        return capi.FD_ACT_RELU
    if isinstance(mod, nn.Hardtanh) and mod.min_val == 0 and mod.max_val == 6:
        return capi.FD_ACT_RELU6
    raise capi.FastDepthError("unsupported activation %r" % (mod,))


def _units(seq):
    """Splits a Sequential (possibly nested) into (conv, bn, act) triples in execution order."""
    flat = []

    def walk(m):
        if isinstance(m, nn.Sequential):
            for c in m:
                walk(c)
        else:
            flat.append(m)
    walk(seq)
    if len(flat) % 3:
        raise capi.FastDepthError("expected Conv-BN-act triples, got %d modules" % len(flat))
    out = []
    for i in range(0, len(flat), 3):
        conv, bn, act = flat[i:i + 3]
        if isinstance(conv, nn.ConvTranspose2d) and isinstance(bn, nn.BatchNorm2d):
            # the one transposed convolution with a kernel (FD_OP_DWT): depthwise, k in {3, 5}, doubling the map (reference models.py:89-99)
            k = conv.kernel_size[0]
            if (conv.bias is not None or conv.kernel_size != (k, k) or k not in (3, 5) or conv.stride != (2, 2) or conv.padding != ((k - 1) // 2,) * 2
                    or conv.output_padding != (1, 1) or conv.dilation != (1, 1) or not conv.groups == conv.in_channels == conv.out_channels):
                raise capi.FastDepthError("transposed conv %r is outside the FastDepth path (only depthwise k in {3, 5}, stride 2, padding (k-1)/2, "
                                          "output_padding 1, no bias, no dilation has a kernel)" % (conv,))
            out.append((conv, bn, _act_of(act)))
            continue
        if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)):
            raise capi.FastDepthError("expected Conv2d, BatchNorm2d, activation; got %r, %r" % (conv, bn))
        if conv.bias is not None or conv.dilation != (1, 1) or conv.padding != (conv.kernel_size[0] // 2,) * 2:
            raise capi.FastDepthError("conv %r is outside the FastDepth path (bias/dilation/padding)" % (conv,))
        out.append((conv, bn, _act_of(act)))
    return out


class Layer:
    __slots__ = ("conv", "bn", "desc", "name")

    def __init__(self, name, conv, bn, act, src, upsample=0, skip=-1, concat=0, op=None):
        # op: told by the walk where the module alone does not say it (the pixel-shuffle and bilinear layers are plain depthwise / pointwise convolutions)
        k = conv.kernel_size[0]
        if op is not None:
            want = (conv.groups == conv.in_channels == conv.out_channels and k in (3, 5)) if op in (capi.FD_OP_DWS, capi.FD_OP_DWB) else (conv.groups == 1 and k == 1)
            if op not in (capi.FD_OP_DWS, capi.FD_OP_PWS, capi.FD_OP_DWB, capi.FD_OP_PWB) or not want or conv.stride != (1, 1):
                raise capi.FastDepthError("%s: conv %r cannot run as op %r" % (name, conv, op))
        elif isinstance(conv, nn.ConvTranspose2d):     # (validated by _units)
            op = capi.FD_OP_DWT
        elif conv.groups == 1 and k == 3 and conv.in_channels == 3 and conv.stride == (2, 2) and src == -1:
            op = capi.FD_OP_STEM
        elif conv.groups == 1 and k in (3, 5) and conv.stride == (1, 1):
            op = capi.FD_OP_CONV       # dense k x k unit of the dense NNConv decoder: the implicit GEMM fd_conv_gemm
        elif conv.groups == conv.in_channels == conv.out_channels and k in (3, 5):
            op = capi.FD_OP_DW
        elif conv.groups == 1 and k == 1:
            op = capi.FD_OP_PW
        else:
            raise capi.FastDepthError("%s: conv %r has no fused kernel on this path" % (name, conv))
        self.name, self.conv, self.bn = name, conv, bn
        self.desc = capi.LayerDesc(op, conv.in_channels, conv.out_channels, k, conv.stride[0], act, src,
                                   upsample, skip, concat)


def _layers_of_plain(model):
    """MobileNet(decoder='nnconv*dw')-shaped module (reference models.py:420-460 + NNConv.forward :244-270): encoder
    `mobilenet.0..13`, decoder `decoder.conv1..6` with a nearest x2 after conv1..conv5 and no skips."""
    layers, src = [], -1
    for i in range(14):
        for j, (conv, bn, act) in enumerate(_units(model.mobilenet[i])):
            layers.append(Layer("mobilenet.%d.%d" % (i, 3 * j), conv, bn, act, src))
            src = len(layers) - 1
    if hasattr(model.decoder, "convt1"):
        # DeConv decoder (reference models.py:145-180): convt1..5 = (transposed depthwise, pointwise), then convf; the transposed layers
        # double the map themselves, so nothing is upsampled
        for name in ["convt%d" % j for j in range(1, 6)] + ["convf"]:
            for q, (conv, bn, act) in enumerate(_units(getattr(model.decoder, name))):
                layers.append(Layer("decoder.%s.%d" % (name, q), conv, bn, act, src))
                src = len(layers) - 1
        return layers
    if hasattr(model.decoder, "conv4") and not hasattr(model.decoder, "conv5") and not hasattr(model.decoder, "conv6"):
        # ShuffleConv decoder (reference models.py:296-333): pixel_shuffle(2) before each of conv1..4 = (depthwise, pointwise) and after conv4.
        # The depthwise layers read through the shuffle, the last pointwise layer writes the network output through it: nothing is upsampled
        for j in range(1, 5):
            units = _units(getattr(model.decoder, "conv%d" % j))
            if len(units) != 2:
                raise capi.FastDepthError("decoder.conv%d: expected a (depthwise, pointwise) pair, got %d units" % (j, len(units)))
            for q, (conv, bn, act) in enumerate(units):
                op = capi.FD_OP_DWS if q == 0 else (capi.FD_OP_PWS if j == 4 else None)
                layers.append(Layer("decoder.conv%d.%d" % (j, q), conv, bn, act, src, op=op))
                src = len(layers) - 1
        return layers
    if getattr(type(model.decoder), "_fd_upsample", "nearest") == "bilinear":
        # BLConv decoder (reference models.py:272-294): NNConv's modules with a bilinear x2 after conv1..conv5.  The interpolation is arithmetic, not
        # an index map: the depthwise layer that follows one does it in registers (FD_OP_DWB), and the last one, which does not commute with conv6's
        # ReLU only, moves behind conv6's affine part (FD_OP_PWB).  conv1.0 sees the encoder output as it is.  Nothing carries `upsample`
        for j in range(1, 7):
            units = _units(getattr(model.decoder, "conv%d" % j))
            if len(units) != (2 if j <= 5 else 1):
                raise capi.FastDepthError("decoder.conv%d: expected %s, got %d units" % (j, "a (depthwise, pointwise) pair" if j <= 5 else "one pointwise unit", len(units)))
            for q, (conv, bn, act) in enumerate(units):
                op = capi.FD_OP_PWB if j == 6 else (capi.FD_OP_DWB if q == 0 and j >= 2 else None)
                layers.append(Layer("decoder.conv%d.%d" % (j, q), conv, bn, act, src, op=op))
                src = len(layers) - 1
        return layers
    pending_up = 0
    for j in range(1, 7):
        for q, (conv, bn, act) in enumerate(_units(getattr(model.decoder, "conv%d" % j))):
            layers.append(Layer("decoder.conv%d.%d" % (j, q), conv, bn, act, src, pending_up, -1))
            pending_up = 0
            src = len(layers) - 1
        pending_up = 1 if j <= 5 else 0
    return layers


def layers_of(model):
    """MobileNetSkipAdd-shaped module -> [Layer].  Skip sources follow models.py:714-719, 724-729.
    A module with `.mobilenet` / `.decoder` (the no-skip sibling) takes the plain walk above."""
    if hasattr(model, "mobilenet") and hasattr(model, "decoder"):
        return _layers_of_plain(model)
    layers, skips = [], {}
    src = -1
    for i in range(14):
        for j, (conv, bn, act) in enumerate(_units(getattr(model, "conv%d" % i))):
            layers.append(Layer("conv%d.%d" % (i, 3 * j), conv, bn, act, src))
            src = len(layers) - 1
        if i in (1, 3, 5):
            skips[i] = src
    skip_after = {2: 5, 3: 3, 4: 1}        # decode stage -> encoder block whose output is added after its upsample
    concat = 1 if getattr(type(model), "_fd_skip", "add") == "concat" else 0      # MobileNetSkipConcat: torch.cat instead of + (models.py:803-808)
    pending_up, pending_skip = 0, -1
    for j in range(1, 7):
        for q, (conv, bn, act) in enumerate(_units(getattr(model, "decode_conv%d" % j))):
            layers.append(Layer("decode_conv%d.%d" % (j, q), conv, bn, act, src, pending_up, pending_skip, concat if pending_skip >= 0 else 0))
            pending_up, pending_skip = 0, -1
            src = len(layers) - 1
        if j <= 5:
            pending_up = 1
            pending_skip = skips[skip_after[j]] if j in skip_after else -1
    return layers
