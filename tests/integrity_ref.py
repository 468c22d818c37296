"""Where the plans write and what stale memory they read: fd_plan and fd_train_plan on poisoned workspaces, with guard bytes around the workspace and around
every caller buffer.  TEST INFRASTRUCTURE ONLY: shared by the CPU tier (tests/test_integrity.py: kind = "emu", the kernels compiled with -DFD_EMU on CPU
tensors) and the GPU tier (tests/test_gpu_integrity.py: kind = "hip", the product library on an MI355X).  Same case tables, seeds and assertions in both.

Nothing here has a tolerance.  The same kernels on the same inputs are deterministic, so
  * everything the caller can see (y, every stored tensor of a KEEP_ACTIVATIONS plan, gradients, running statistics, num_batches_tracked) agrees BIT FOR BIT
    whether the workspace started as 0x00 bytes, 0xFF bytes (a NaN in fp32 / fp16 / bf16, -1 in every integer slot), 0x7B bytes (finite and large: 1.3e36 in
    fp32 and bf16, 6.1e4 in fp16, 8.9e18 in an int64) or 0xA5 bytes: a kernel that reads a word nobody wrote shows up as a difference, and the 0x7B fill tells
    "multiplies stale memory by zero" (differs under 0xFF only) from "uses it" (differs under 0x7B too);
  * the guard bytes (GUARD = 4096 of the fill in front of and behind the workspace, >= 64 bytes of 0xA5 before, between and behind x, y, dy, every parameter, running
    statistic and gradient tensor) are untouched, the read-only inputs unchanged, and the alignment padding behind every stored tensor still holds the fill;
  * with the gradient tensors back to back at the offsets of the product's flat gradient buffer every gradient is bit-equal to the guarded layout's."""
import ctypes
import functools
import re
import time

import numpy as np
import torch

import forms
import harness
from fastdepth_hip import capi
from oracle import inputs

F = capi
FILLS = (0x00, 0xFF, 0x7B, 0xA5)
GUARD = 4096
H16 = (torch.float16, torch.bfloat16)


def _dt(dtype):
    return str(dtype).split(".")[-1]


# ---- models -----------------------------------------------------------------------------------------------------------------------------

# TINY with 32 channels into conv12.0 (stride 2) and conv13.0: the units on the 1 x 1 map of a 32 x 32 input whose channel count the register-window train
# kernels accept (C / 4 a power of two in 8 ... 64) -- at batch 3 their tensors are 3 x 1 x 1 x 32 floats = 384 bytes, off a 256-byte boundary
ROWS32 = ((8, 16, 24, 24, 32, 32, 40, 40, 40, 40, 40, 32, 32, 48), forms.TINY[1])
WIDTHS = {"tiny": forms.TINY, "ragged": forms.RAGGED, "wide": forms.WIDE, "units": forms.UNITS, "g16": forms.G16, "rows32": ROWS32}
SIBLING_SHAPE = (2, 32, 32)          # the smallest shape of tests/test_deconv.py, test_shuffle.py, test_bilinear.py (and of the no-skip / skip-concat checks: 32 x 32)


@functools.lru_cache(maxsize=None)
def model_of(name):
    """The module of a case, built once, shared by every case and both tiers, never modified (plans work on private copies of the parameters)."""
    models = inputs.product_models()
    if name in WIDTHS:
        # (seed 24: the prediction of every one of these networks is positive nearly everywhere at the shapes below -- seed 21, which tests/forms.py uses,
        # leaves the head of TINY, RAGGED and WIDE below zero everywhere at these shapes; `alive` below asserts it)
        return forms.small_model(WIDTHS[name][0], WIDTHS[name][1], seed=24)
    if name == "noskip":
        torch.manual_seed(23)
        return harness.randomize_bn(models.MobileNet("nnconv5dw", (32, 32), pretrained=False), 24)
    if name == "skipconcat":
        torch.manual_seed(31)
        return harness.randomize_bn(models.MobileNetSkipConcat((32, 32), pretrained=False), 32)
    if name == "skipconcat_small":          # the widths of forms.check_skip_concat_train_step_layer_local
        torch.manual_seed(41)
        enc = (8, 32, 24, 32, 32, 32, 40, 40, 40, 40, 40, 40, 48, 48)
        return harness.randomize_bn(models.MobileNetSkipConcat((64, 64), pretrained=False, channels=(enc, (40, 32, 32, 32, 8, 1))), 42)
    import bilinear_ref
    import deconv_ref
    import shuffle_ref
    for ref in (deconv_ref, shuffle_ref, bilinear_ref):
        if name in ref.DECODERS:
            return ref.case(name, SIBLING_SHAPE)[0]
    raise KeyError(name)


def alive(y_bits):
    """share of the prediction's pixels above zero: an all-zero prediction (a head whose BatchNorm shift is below zero everywhere) would compare equal whatever
    the layers before it did"""
    return float((y_bits.view(np.float32) > 0).mean())


def input_of(shape, seed=77):
    return torch.rand(shape[0], 3, shape[1], shape[2], generator=torch.Generator().manual_seed(seed))


# ---- kernel families --------------------------------------------------------------------------------------------------------------------

def family(info, dtype=None):
    """The kernel plan.info() names for a layer, as it names it (dw3_rows8 apart from dw3_rows; pw_gemm apart by the plan's dtype: fd_pw_gemm_f32 and
    fd_pw_gemm_h16 are different kernels with different store paths).  None: the layer has no kernel and no tensor of its own."""
    if info.startswith("(fused into"):
        return None
    if info.startswith("(dw "):
        return "epilogue_dw"                  # a depthwise layer written by its producer's pw_gemm16 epilogue
    if info.startswith("(pointwise head"):
        return "fused_head"                   # the head evaluated on a producer's accumulators / output tile: that kernel writes y
    name = re.split(r"[<\s]", info)[0]
    if name == "pw_gemm" and dtype is not None:
        return "pw_gemm_f32" if dtype == torch.float32 else "pw_gemm_h16"
    return name


INFER_FAMILIES = ("stem3x3s2", "dw3_rows", "dw3_rows8", "dwconv", "dw5_rows", "pw_gemm_f32", "pw_gemm_h16", "pw_gemm16", "dwpw", "epilogue_dw", "fused_head", "head_pw1", "dwt_rows", "dws_rows",
                  "head_shuffle", "dwb_rows", "head_bilinear")
# Families no case can catch with a tensor that ends off a 256-byte boundary or with a caller buffer, and why.
UNPADDABLE = {
    # the stem's output is B x H/2 x W/2 x C elements with H % 32 == W % 32 == 0 (fd_plan_create) and C % 8 == 0 (the 4-channel store lanes of fd_stem3x3s2):
    # (H/2)(W/2) is a multiple of 256, so the tensor is a multiple of 256 x 8 x 2 bytes in every plan; it writes no caller buffer
    "stem3x3s2": "B*(H/2)*(W/2)*C*esz with (H/2)*(W/2) % 256 == 0",
    # fd_dw5_rows runs the 5x5 units on up2(low) + skip of a 16-bit plan only (decode_conv3 / 4 / 5: maps of 1/8, 1/4, 1/2 of the input), so h*w % 16 == 0, and a
    # 16-bit plan has C % 8 == 0: B*h*w*C*2 bytes is a multiple of 16 x 8 x 2 = 256.  (Tensors that end off a boundary exist on the 1/16 and 1/32 maps only.)
    "dw5_rows": "B*h*w*C*2 with h*w % 16 == 0 and C % 8 == 0",
    # the DeConv / ShuffleConv / BLConv siblings exist at full width only (models.MobileNet takes no channel list).  At 32 x 32, the smallest input a plan
    # accepts, their transposed / pixel-shuffle / bilinear units write h x w x C = 2x2x1024, 4x4x512, ... 32x32x64 (DeConv), 2x2x256, 4x4x64, 8x8x16, 16x16x4
    # (ShuffleConv), 2x2x512 ... 16x16x64 (BLConv): at least 1024 elements per frame, all powers of two; a larger input multiplies h*w by (H/32)(W/32).
    # So every such tensor is a multiple of 1024 x 2 bytes.  Their heads (head_shuffle, head_bilinear) write y and are covered by its guards.
    "dwt_rows": "h*w*C a multiple of 1024 elements per frame", "dws_rows": "h*w*C a multiple of 1024 elements per frame", "dwb_rows": "h*w*C a multiple of 1024 elements per frame",
}


# ---- inference --------------------------------------------------------------------------------------------------------------------------

def _infer_flags(dtype):
    out = [("default", 0), ("gemm16", F.FD_TUNE_FORCE_GEMM16)]
    out.append(("unit_fusion", F.FD_TUNE_FORCE_UNIT_FUSION) if dtype == torch.float32 else ("epilogue_fusion", F.FD_TUNE_FORCE_EPILOGUE_FUSION))
    out.append(("fallbacks", F.FD_PLAN_NO_GEMM16 | F.FD_PLAN_NO_EPILOGUE_FUSION | F.FD_PLAN_NO_ROWS8))
    out.append(("dw_h8", F.FD_TUNE_FORCE_DW_H8 | F.FD_TUNE_NO_DW5_ROWS))
    return out


def _infer_table():
    """(id, model, (b, h, w), dtype, flags, keep, emulator tier: False = runs, True = runs marked slow, None = device tier only -- a forward of a full-width
    sibling takes the emulator about as long as the whole device tier takes the MI355X).  Batches 1 and 3 on 32 x 32, 32 x 96 and 64 x 96 inputs: the deep maps are 1 x 1 to 2 x 3
    pixels, so most tensors of B x h x w x C x esz bytes end off a 256-byte boundary; UNITS at the two smallest shapes at which fd_dwpw_f32 is selected.
    Every model runs in every dtype with every flag set of _infer_flags; no-keep plans with the flag sets that change what a no-keep plan does."""
    shapes = {"tiny": [(3, 32, 96)], "ragged": [(1, 64, 96)], "wide": [(3, 32, 32)], "units": [(2, 64, 64), (1, 96, 160)]}
    cases = []
    for model in ("tiny", "ragged", "wide", "units"):
        for shape in shapes[model]:
            for dtype in (torch.float32, torch.float16, torch.bfloat16):
                for fname, flags in _infer_flags(dtype):
                    # UNITS beyond fd_dwpw_f32 (the fp32 default and unit-fusion plans): its 16-bit plans and the other flag sets run on the device tier only
                    units_device_only = model == "units" and (dtype != torch.float32 or fname not in ("default", "unit_fusion"))
                    for keep in (True, False):
                        if not keep and fname not in ("default", "unit_fusion", "epilogue_fusion"):
                            continue                              # no-keep: the lifetime arena and the fusions only a no-keep plan takes (the head on a producer's tile)
                        cid = "%s-%dx%dx%d-%s-%s-%s" % (model, shape[0], shape[1], shape[2], _dt(dtype), fname, "keep" if keep else "nokeep")
                        slow = not (model in ("tiny", "ragged") and (keep or fname == "default")) and not (model == "units" and shape == (2, 64, 64))
                        if slow and not (keep and (dtype == torch.float32 or fname == "default")):
                            slow = None
                        if units_device_only:
                            slow = None
                        cases.append((cid, model, shape, dtype, flags, keep, slow))
    for model in ("noskip", "skipconcat", "deconv5dw", "deconv3dw", "shuffle5dw", "shuffle3dw", "blconv5dw", "blconv3dw"):
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            for keep in ((True, False) if dtype == torch.float32 else (True,)):
                cid = "%s-%dx%dx%d-%s-default-%s" % ((model,) + SIBLING_SHAPE + (_dt(dtype), "keep" if keep else "nokeep"))
                cases.append((cid, model, SIBLING_SHAPE, dtype, 0, keep, True if (keep and dtype == torch.float32) else None))
    return cases


INFER_CASES = _infer_table()


def _infer_run(kind, m, x, dtype, flags, keep, fill, bundle=None):
    """One plan on a workspace of `fill` bytes, one guarded forward: ({tensor name: bytes}, info, figures)."""
    cp = harness.CPlan(kind, m, x, keep=keep, dtype=dtype, flags=flags, fill=fill, guard=GUARD, bundle=bundle)
    try:
        info = cp.info()
        y = cp.forward(x, guarded=True)
        out = {}                                                  # in layer order, the prediction last: the first difference names the first layer that differs
        fig = {"guards_bad": cp.bad_guards(), "guard_bytes": cp.ws.numel() - cp.nbytes + cp.io.guard_bytes, "x_changed": int(not np.array_equal(harness.bits_of(cp.io.view("x")), harness.bits_of(x))),
               "pad_bytes": 0, "pad_bad": [], "where": cp.io.first_bad_guard()}
        if keep:
            for i in range(len(info)):
                r = cp.raw(i)
                if r is None:
                    continue
                out["layer%d" % i] = r[0]
                fig["pad_bytes"] += len(r[1])
                bad = np.nonzero(r[1] != fill)[0]
                if len(bad):
                    fig["pad_bad"].append("layer %d (%s): %d padding bytes changed, first %d bytes behind the tensor's end" % (i, info[i], len(bad), int(bad[0])))
        out["y"] = harness.bits_of(y)
        return out, info, fig
    finally:
        cp.close()


def _first_difference(ref, got, info):
    for k in ref:
        if not np.array_equal(ref[k], got[k]):
            i = int(k[5:]) if k.startswith("layer") else len(info) - 1
            return "%s (%s): %d of %d bytes differ" % (k, info[i], int((ref[k] != got[k]).sum()), len(ref[k]))
    return None


def check_inference_plan(kind, cid, model, shape, dtype, flags, keep):
    """Sections 2 and 3 for one inference plan: y (and every fd_layer_output tensor of a keep plan) bit-equal across the four fills; workspace and caller
    guards untouched, x unchanged, the alignment padding behind every stored tensor still the fill -- under every fill."""
    t0 = time.time()
    m = model_of(model).eval()
    x = input_of(shape).to(forms.device_of(kind))
    runs = {fill: _infer_run(kind, m, x, dtype, flags, keep, fill) for fill in FILLS}
    ref, info, _ = runs[FILLS[0]]
    assert not np.isnan(ref["y"].view(np.float32)).any() and alive(ref["y"]) > 0.2, "the clean run's prediction holds a NaN or is dead: %.2f of it above zero" % alive(ref["y"])
    differ = {"%#04x" % fill: _first_difference(ref, runs[fill][0], info) for fill in FILLS[1:]}
    differ = {k: v for k, v in differ.items() if v}
    figs = [runs[fill][2] for fill in FILLS]
    forms.note(kind, "inference_plan", cid, t0, fills="/".join("%#04x" % f for f in FILLS), tensors=len(ref), fills_that_differ=",".join(differ) or "none",
               guard_bytes=figs[0]["guard_bytes"], padding_bytes=figs[0]["pad_bytes"], bytes_touched=sum(f["guards_bad"] + len(f["pad_bad"]) for f in figs))
    assert not differ, "results depend on what the workspace held: %s" % differ
    for fill, f in zip(FILLS, figs):
        assert f["guards_bad"] == 0, "fill %#04x: %d guard bytes changed, first near %s" % (fill, f["guards_bad"], f["where"])
        assert f["x_changed"] == 0, "fill %#04x: the network input was modified" % fill
        assert not f["pad_bad"], "fill %#04x: %s" % (fill, f["pad_bad"])


INFER_REUSE_CASES = [c for c in INFER_CASES if c[0] in ("tiny-3x32x96-float32-default-nokeep", "tiny-3x32x96-float16-epilogue_fusion-keep", "ragged-1x64x96-bfloat16-default-nokeep",
                                                     "units-2x64x64-float32-unit_fusion-nokeep")]


def check_inference_plan_reuse(kind, cid, model, shape, dtype, flags, keep):
    """One plan runs input A = 1e3 x, then B = x: B's results are a fresh plan's, bit for bit (nothing of A survives in the workspace: stream-K counters, LDS-DMA
    rings' flags, fused tiles)."""
    t0 = time.time()
    m = model_of(model).eval()
    x = input_of(shape).to(forms.device_of(kind))
    want, info, _ = _infer_run(kind, m, x, dtype, flags, keep, 0xFF)
    cp = harness.CPlan(kind, m, x, keep=keep, dtype=dtype, flags=flags, fill=0xFF, guard=GUARD)
    try:
        ya = harness.bits_of(cp.forward(x * 1e3, guarded=True))
        yb = harness.bits_of(cp.forward(x, guarded=True))
        got = {"layer%d" % i: cp.raw(i)[0] for i in range(len(info)) if cp.raw(i) is not None} if keep else {}
        got["y"] = yb
        bad = cp.bad_guards()
    finally:
        cp.close()
    d = _first_difference(want, got, info)
    forms.note(kind, "inference_plan_reuse", cid, t0, tensors=len(want), differs=d or "none", a_differs_from_b=int(not np.array_equal(ya, want["y"])), guards_bad=bad)
    assert not np.array_equal(ya, want["y"]), "input A gave input B's prediction: the case checks nothing"
    assert d is None and bad == 0, d


BUNDLE_CASES = [("tiny", (3, 32, 96), torch.float32), ("ragged", (1, 64, 96), torch.float16), ("wide", (3, 32, 32), torch.bfloat16)]


def check_bundle_round_trip(kind, model, shape, dtype):
    """export -> fd_plan_import -> a 0xFF workspace -> fd_plan_import_weights -> forward: the source plan's prediction bit for bit, guards untouched."""
    t0 = time.time()
    m = model_of(model).eval()
    x = input_of(shape).to(forms.device_of(kind))
    src = harness.CPlan(kind, m, x, keep=False, dtype=dtype, fill=0x00, guard=GUARD)
    try:
        want = harness.bits_of(src.forward(x, guarded=True))
        blob = src.export()
    finally:
        src.close()
    got, _, fig = _infer_run(kind, m, x, dtype, 0, False, 0xFF, bundle=blob)
    forms.note(kind, "bundle_round_trip", "%s-%s" % (model, _dt(dtype)), t0, bundle_bytes=len(blob), bytes_that_differ=int((got["y"] != want).sum()), guards_bad=fig["guards_bad"])
    assert np.array_equal(got["y"], want) and fig["guards_bad"] == 0 and fig["x_changed"] == 0


def family_coverage(kind, cases=None):
    """{family: number of (case, tensor) pairs in which a kernel of that family writes a stored tensor that ends off a 256-byte boundary (keep plans: the padding
    behind it is checked) or writes the caller's y (every plan: the guards around y are checked)} over INFER_CASES.  From the plans alone: nothing is launched."""
    count = {f: 0 for f in INFER_FAMILIES}
    dev = forms.device_of(kind)
    for cid, model, shape, dtype, flags, keep, _ in (cases or INFER_CASES):
        x = input_of(shape).to(dev)
        cp = harness.CPlan(kind, model_of(model).eval(), x, keep=keep, dtype=dtype, flags=flags, pack=False)
        try:
            info = cp.info()
            for i, s in enumerate(info):
                fam = family(s, dtype)
                if fam is None:
                    continue
                assert fam in count, "a kernel family the table does not know: %s" % s
                if fam.startswith("head_") or fam == "fused_head":
                    count[fam] += 1                                   # writes y
                    continue
                if " head on " in s:
                    count[fam] += 1                                   # ... and so does the kernel that evaluates a fused head
                r = cp.raw(i) if keep else None
                if r is not None and len(r[1]):
                    count[fam] += 1
        finally:
            cp.close()
    return count


def check_family_coverage(kind):
    t0 = time.time()
    count = family_coverage(kind)
    forms.note(kind, "family_coverage", "inference", t0, **count)
    missing = [f for f in INFER_FAMILIES if not count[f] and f not in UNPADDABLE]
    assert not missing, "no case of the table catches these families with a padded tensor or a caller buffer: %s" % missing
    assert all(count[f] == 0 for f in UNPADDABLE), "an exception of the table is no exception: %s" % count


# ---- train step -------------------------------------------------------------------------------------------------------------------------

# (id, model, (b, h, w), dtype, flags, keep, emulator tier: False = runs, True = runs marked slow, None = device tier only)
TRAIN_CASES = [
    ("tiny-3x32x32-float32-default-keep", "tiny", (3, 32, 32), torch.float32, 0, True, False),
    ("tiny-2x32x96-bfloat16-default-keep", "tiny", (2, 32, 96), torch.bfloat16, 0, True, False),
    ("ragged-3x32x32-bfloat16-default-keep", "ragged", (3, 32, 32), torch.bfloat16, 0, True, False),
    ("ragged-2x32x96-float32-default-nokeep", "ragged", (2, 32, 96), torch.float32, 0, False, False),
    ("g16-3x32x32-float32-gemm16-keep", "g16", (3, 32, 32), torch.float32, F.FD_TUNE_FORCE_GEMM16, True, False),
    ("skipconcat-2x32x32-float32-default-keep", "skipconcat_small", (2, 32, 32), torch.float32, 0, True, False),
    ("skipconcat-3x32x32-bfloat16-default-keep", "skipconcat_small", (3, 32, 32), torch.bfloat16, 0, True, False),
    ("tiny-3x32x32-float32-dw_bwd1-keep", "tiny", (3, 32, 32), torch.float32, F.FD_TUNE_DW_BWD1, True, False),
    ("ragged-2x32x96-bfloat16-dw_bwd1-keep", "ragged", (2, 32, 96), torch.bfloat16, F.FD_TUNE_DW_BWD1, True, False),
    ("tiny-2x32x96-float32-no_consumer_finalize-keep", "tiny", (2, 32, 96), torch.float32, F.FD_TUNE_NO_CONSUMER_FINALIZE, True, False),
    ("ragged-3x32x32-bfloat16-no_consumer_finalize-nokeep", "ragged", (3, 32, 32), torch.bfloat16, F.FD_TUNE_NO_CONSUMER_FINALIZE, False, False),
    ("tiny-3x32x32-bfloat16-no_pw_pairing-keep", "tiny", (3, 32, 32), torch.bfloat16, F.FD_TUNE_NO_PW_PAIRING, True, False),
    # 224 x 32: map heights 112 ... 7, 8-row tiles with a ragged last tile in 16-channel blocks (forms.TRAIN_LOCAL_CASES "tiny_tall")
    ("tiny_tall-2x224x32-float32-dw_th8_cb16-keep", "tiny", (2, 224, 32), torch.float32, F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16, True, True),
    ("tiny_tall-2x224x32-bfloat16-dw_th8_cb16-keep", "tiny", (2, 224, 32), torch.bfloat16, F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16, True, None),
    ("g16-2x32x96-float32-gemm16_no_consumer_finalize-nokeep", "g16", (2, 32, 96), torch.float32, F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_NO_CONSUMER_FINALIZE, False, True),
    ("ragged-3x32x32-float32-dw_bwd1-nokeep", "ragged", (3, 32, 32), torch.float32, F.FD_TUNE_DW_BWD1, False, True),
    ("ragged-2x32x96-bfloat16-no_pw_pairing-keep", "ragged", (2, 32, 96), torch.bfloat16, F.FD_TUNE_NO_PW_PAIRING, True, True),
    ("skipconcat-2x32x96-bfloat16-dw_bwd1-keep", "skipconcat_small", (2, 32, 96), torch.bfloat16, F.FD_TUNE_DW_BWD1, True, None),
    # G16 in 16 bits: the packed 16-bit operand copies ([N][K64], [K][N64]) of 96- and 160-channel units, a ragged last 64-column tile in both GEMMs
    ("g16-3x32x32-bfloat16-default-keep", "g16", (3, 32, 32), torch.bfloat16, 0, True, True),
    ("g16-2x32x96-bfloat16-no_pw_pairing-nokeep", "g16", (2, 32, 96), torch.bfloat16, F.FD_TUNE_NO_PW_PAIRING, False, None),
    # the forms the flags above do not select at these sizes (check_train_coverage): the register-window kernels (fd_dw3_rows_train, fd_dw3s2_dgrad_rows +
    # fd_dw3_wgrad_rows: by default on maps of >= 28 x 28 only, whose tensors are multiples of 256 bytes) on the 32-channel units of ROWS32, conv12.0 and
    # conv13.0 with a 1 x 1 output (3 x 1 x 1 x 32 floats = 384 bytes); every backward kernel on its own (fd_dw_wgrad + fd_dw_dgrad, fd_pw_wgrad_f32 + fd_pw_dgrad_f32);
    # the 16-bit BatchNorm-backward apply pass without the in-kernel finalisation (fd_bn_bwd_apply_h16) in a keep plan
    ("rows32-3x32x32-float32-dw_force_rows-keep", "rows32", (3, 32, 32), torch.float32, F.FD_TUNE_DW_FORCE_ROWS, True, True),
    ("ragged-3x32x32-float32-no_bwd_pairing-keep", "ragged", (3, 32, 32), torch.float32, F.FD_PLAN_NO_BWD_PAIRING, True, True),
    ("tiny-3x32x32-bfloat16-no_consumer_finalize-keep", "tiny", (3, 32, 32), torch.bfloat16, F.FD_TUNE_NO_CONSUMER_FINALIZE, True, None),
]
WHICH = {0: "z", 1: "G", 2: "bn_table", 3: "skip_grad", 4: "dz"}
READ_ONLY = ("conv_weight", "bn_weight", "bn_bias")


def _train_inputs(shape):
    g = torch.Generator().manual_seed(9)
    x = torch.rand(shape[0], 3, shape[1], shape[2], generator=g)
    target = 2.0 + torch.rand(shape[0], 1, shape[1], shape[2], generator=g)
    return x, target


def _train_step(tp, x, target, keep, fill):
    """One forward + backward on `tp` -> ({name: bytes}, figures)."""
    dev = tp.dev
    before = [{k: harness.bits_of(d[k]) for k in READ_ONLY} for d in tp.tensors]
    y = tp.forward(x.to(dev))
    dy = torch.sign(y.cpu() - target) / y.numel()
    grads = tp.backward(dy)
    out = {}                     # the stored tensors in layer order first (filled below), then what the caller sees: the first difference names the first unit that differs
    if keep:
        for i in range(tp.n):
            for which, nm in WHICH.items():
                r = tp.raw(i, which)
                if r is not None:
                    out["%s %d" % (nm, i)] = r[0]
    out.update({"y": harness.bits_of(y), "num_batches_tracked": harness.bits_of(tp.nbt)})
    for i, (g, d) in enumerate(zip(grads, tp.tensors)):
        for k in READ_ONLY:
            out["grad %d %s" % (i, k)] = harness.bits_of(g[k])
        out["running_mean %d" % i], out["running_var %d" % i] = harness.bits_of(d["bn_mean"]), harness.bits_of(d["bn_var"])
    fig = {"guards_bad": tp.bad_guards(), "guard_bytes": tp.guard_bytes(), "pad_bytes": 0, "pad_bad": [],
           "where": [a.first_bad_guard() for a in (tp.pa, tp.ga, tp.io, tp.dio) if a.first_bad_guard()],
           "inputs_changed": [n for n, a, b in [("x", tp.io.view("x"), x), ("dy", tp.dio.view("dy"), dy)] if not np.array_equal(harness.bits_of(a), harness.bits_of(b))] +
                             ["%s %d" % (k, i) for i, d in enumerate(tp.tensors) for k in READ_ONLY if not np.array_equal(harness.bits_of(d[k]), before[i][k])]}
    if keep:
        for i in range(tp.n):
            for which, nm in WHICH.items():
                r = tp.raw(i, which)
                if r is None:
                    continue
                fig["pad_bytes"] += len(r[1])
                bad = np.nonzero(r[1] != fill)[0]
                if len(bad):
                    fig["pad_bad"].append("%s of layer %d (%s): %d padding bytes changed, first %d bytes behind the tensor's end" % (nm, i, tp.layers[i].name, len(bad), int(bad[0])))
    return out, fig


def _train_run(kind, m, x, target, dtype, flags, keep, fill, layout):
    tp = harness.CTrainPlan(kind, m, x.to(forms.device_of(kind)), keep=keep, dtype=dtype, flags=flags, fill=fill, guard=GUARD, layout=layout)
    try:
        return _train_step(tp, x, target, keep, fill)
    finally:
        tp.close()


def _first_train_difference(ref, got, layers):
    for k in ref:
        if not np.array_equal(ref[k], got[k]):
            i = k.split()[1] if " " in k else None
            return "%s%s: %d of %d bytes differ" % (k, " (%s)" % layers[int(i)].name if i is not None and i.isdigit() else "", int((ref[k] != got[k]).sum()), len(ref[k]))
    return None


def check_train_plan(kind, cid, model, shape, dtype, flags, keep):
    """Sections 2 and 3 for one train step: y, all gradients, the updated running statistics, num_batches_tracked (and, keep plans, every tensor
    fd_train_layer_tensor exposes) bit-equal across the fills; guards around the workspace and around / between x, y, dy, every parameter, running statistic
    and gradient untouched; x, dy and the parameters unchanged; padding behind the stored tensors still the fill.  The 0xA5 run lays the gradients back to
    back at the offsets of the product's flat gradient buffer: bit-equal gradients, and the (up to 3) padding elements behind a tensor untouched."""
    t0 = time.time()
    m = model_of(model).train()
    layers = harness.layers_of(m)
    x, target = _train_inputs(shape)
    runs = {fill: _train_run(kind, m, x, target, dtype, flags, keep, fill, "flat" if fill == 0xA5 else "guarded") for fill in FILLS}
    ref = runs[FILLS[0]][0]
    assert not np.isnan(ref["y"].view(np.float32)).any() and not any(np.isnan(v.view(np.float32)).any() for k, v in ref.items() if k.startswith("grad")), "the clean step holds a NaN"
    assert (ref["num_batches_tracked"].view(np.int64) == 1).all() and alive(ref["y"]) > 0.2, alive(ref["y"])
    differ = {"%#04x" % fill: _first_train_difference(ref, runs[fill][0], layers) for fill in FILLS[1:]}
    differ = {k: v for k, v in differ.items() if v}
    figs = [runs[fill][1] for fill in FILLS]
    forms.note(kind, "train_plan", cid, t0, fills="/".join("%#04x" % f for f in FILLS), tensors=len(ref), fills_that_differ=",".join(differ) or "none",
               guard_bytes=figs[0]["guard_bytes"], flat_layout_guard_bytes=figs[-1]["guard_bytes"], padding_bytes=figs[0]["pad_bytes"],
               bytes_touched=sum(f["guards_bad"] + len(f["pad_bad"]) for f in figs))
    assert not differ, "results depend on what the workspace held (0xa5: gradients back to back): %s" % differ
    for fill, f in zip(FILLS, figs):
        assert f["guards_bad"] == 0, "fill %#04x: %d guard bytes changed, first near %s" % (fill, f["guards_bad"], f["where"])
        assert not f["inputs_changed"], "fill %#04x: read-only inputs were modified: %s" % (fill, f["inputs_changed"])
        assert not f["pad_bad"], "fill %#04x: %s" % (fill, f["pad_bad"])


TRAIN_REUSE_CASES = [c for c in TRAIN_CASES if c[0] in ("tiny-3x32x32-float32-default-keep", "ragged-3x32x32-bfloat16-default-keep")]


def check_train_plan_reuse(kind, cid, model, shape, dtype, flags, keep):
    """A step on A = 1e3 x (finite, other statistics bins: fd_stat_add picks the accumulator by the binary exponent), parameters, running statistics and
    num_batches_tracked restored, then a step on x: a fresh plan's step on x, bit for bit (the mechanics of check_clean_step_after_poison)."""
    t0 = time.time()
    m = model_of(model).train()
    x, target = _train_inputs(shape)
    want, _ = _train_run(kind, m, x, target, dtype, flags, keep, 0xFF, "guarded")
    tp = harness.CTrainPlan(kind, m, x.to(forms.device_of(kind)), keep=keep, dtype=dtype, flags=flags, fill=0xFF, guard=GUARD, layout="guarded")
    try:
        init = [{k: v.clone() for k, v in d.items()} for d in tp.tensors]
        a, _ = _train_step(tp, x * 1e3, target, keep, 0xFF)
        for d, d0 in zip(tp.tensors, init):
            for k in d:
                d[k].copy_(d0[k])
        tp.nbt.zero_()
        got, fig = _train_step(tp, x, target, keep, 0xFF)
    finally:
        tp.close()
    d = _first_train_difference(want, got, harness.layers_of(m))
    forms.note(kind, "train_plan_reuse", cid, t0, tensors=len(want), differs=d or "none", a_differs_from_b=int(not np.array_equal(a["y"], want["y"])), guards_bad=fig["guards_bad"])
    assert not np.array_equal(a["y"], want["y"]) and not np.array_equal(a["running_mean 0"], want["running_mean 0"]), "step A equals step B: the case checks nothing"
    assert d is None and fig["guards_bad"] == 0, d


# ---- which train kernels the train cases reach -------------------------------------------------------------------------------------------

# Every kernel fd_train_forward / fd_train_backward can launch (the FD_LAUNCH sites of csrc/fd_train_impl.h and csrc/fd_train_bwd_impl.h).
TRAIN_KERNELS = ("fd_pack_train_w_h16", "fd_stem_train", "fd_dw5_rows_train", "fd_dw3_rows_fwd", "fd_dw3_rows_train", "fd_dwconv_train", "fd_head_train", "fd_pw_gemm16_f32",
                 "fd_pw_gemm_train_f32", "fd_pw_gemm_train_h16", "fd_bn_finalize_rows_f32", "fd_head_apply_f32",
                 "fd_head_bwd_reduce_f32", "fd_head_bwd", "fd_bn_bwd_finalize_rows_f32", "fd_reduce_weights_batch_f32", "fd_dw_wgrad", "fd_dw_dgrad", "fd_dw5_bwd_rows", "fd_dw3_bwd_rows",
                 "fd_dw3s2_bwd_rows", "fd_dw3s2_dgrad_rows", "fd_dw3_wgrad_rows", "fd_dw_bwd1", "fd_dw_bwd", "fd_bn_bwd_apply_fin_h16", "fd_bn_bwd_apply_h16", "fd_pw_bwd_h16",
                 "fd_pw_wgrad_h16", "fd_pw_dgrad_h16", "fd_pw_bwd_f32", "fd_pw_wgrad_f32", "fd_pw_dgrad_f32", "fd_stem_wgrad_rows", "fd_stem_wgrad")
# The kernels that store into a caller buffer themselves (every launch of them is between guard bytes, whatever the shapes)
TRAIN_CALLER_WRITERS = {
    "fd_head_apply_f32": "y",
    "fd_bn_finalize_rows_f32": "running_mean, running_var, num_batches_tracked (fd_bn_fin)",
    "fd_bn_bwd_finalize_rows_f32": "the bn_weight / bn_bias gradients (fd_bn_bwd_fin)",
    "fd_reduce_weights_batch_f32": "every conv_weight gradient (fd_wred_args::out)",
}
# What the plan's test hooks (csrc/fd_tuning.h: fd_train_plan_unit_kernels) tell of a unit without a launch: the emulator tier's census, and the device's too
TRAIN_FORMS = ("stem", "head", "pw_gemm_train", "pw_gemm16_train", "dw_fwd_tiled_or_regwin", "dw_fwd_rows5", "dw_fwd_rows3", "dw_bwd_tiled_or_regwin", "dw_bwd_rows",
               "finalised_by_consumer", "bwd_finalised_in_kernel")


def _unit_forms(tp, i):
    d = tp.layers[i].desc
    bits = tp.lib.fd_train_plan_unit_kernels(tp.h, i)
    assert bits >= 0
    out = ["finalised_by_consumer"] if bits & 2 else []
    out += ["bwd_finalised_in_kernel"] if bits & 4 else []
    if d.op == capi.FD_OP_STEM:
        return out + ["stem"]
    if d.op == capi.FD_OP_PW:
        return out + ["head" if d.cout == 1 else "pw_gemm16_train" if bits & 1 else "pw_gemm_train"]
    return out + ["dw_fwd_rows5" if bits & 16 else "dw_fwd_rows3" if bits & 32 else "dw_fwd_tiled_or_regwin", "dw_bwd_rows" if bits & 8 else "dw_bwd_tiled_or_regwin"]


def _padded_units(tp):
    """The units of a KEEP plan around which the padding check is live: an activation-sized tensor fd_train_layer_tensor exposes for the unit, for its
    producer or for its skip source (what the unit's kernels read and write: z, G, the skip gradient, dz) ends off a 256-byte boundary.  (The [4][C] BatchNorm
    table does so for nearly every unit, whatever the map's size: it is checked, but does not count here.)"""
    own = [any(r is not None and len(r[1]) for r in (tp.raw(i, which) for which in WHICH if which != 2)) for i in range(tp.n)]
    return {i for i in range(tp.n) if own[i] or any(j >= 0 and own[j] for j in (tp.layers[i].desc.src, tp.layers[i].desc.skip))}


def train_census(kind):
    """({form: count}, {kernel: count}, {kernel: launches}) over the TRAIN_CASES this tier runs.  A unit of a keep plan counts for its forms when it is one of _padded_units.
    Device tier only (the launch trace of fd_trace_begin / fd_trace_end, one step per case): a launch counts for its kernel when it is recorded for such a
    unit, or when the kernel is one of TRAIN_CALLER_WRITERS (any plan)."""
    forms_n, kernels_n, launched = {f: 0 for f in TRAIN_FORMS}, {k: 0 for k in TRAIN_KERNELS}, {k: 0 for k in TRAIN_KERNELS}
    dev = forms.device_of(kind)
    for cid, model, shape, dtype, flags, keep, emu in TRAIN_CASES:
        if kind == "emu" and emu is None:
            continue
        m = model_of(model).train()
        x, target = _train_inputs(shape)
        tp = harness.CTrainPlan(kind, m, x.to(dev), keep=keep, dtype=dtype, flags=flags, fill=0xA5, guard=GUARD, layout="guarded")
        try:
            tp.lib.fd_train_plan_unit_kernels.restype, tp.lib.fd_train_plan_unit_kernels.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]
            padded = _padded_units(tp) if keep else set()
            for i in padded:
                for f in _unit_forms(tp, i):
                    forms_n[f] += 1
            if kind != "hip":
                continue
            capi.check(tp.lib, tp.lib.fd_trace_begin(), "fd_trace_begin")
            y = tp.forward(x.to(dev)).cpu()
            tp.backward(torch.sign(y - target) / y.numel())
            n, recs = ctypes.c_int32(), (capi.TraceRecord * 4096)()
            capi.check(tp.lib, tp.lib.fd_trace_end(tp.stream, recs, 4096, ctypes.byref(n)), "fd_trace_end")
            assert 0 < n.value <= 4096 and tp.bad_guards() == 0
            for r in recs[:n.value]:
                k = re.match(r"\(*\s*(fd_\w+)", r.kernel.decode()).group(1)
                assert k in kernels_n, "a train kernel the table does not know: %s" % r.kernel.decode()
                launched[k] += 1
                if k in TRAIN_CALLER_WRITERS or r.layer in padded:
                    kernels_n[k] += 1
        finally:
            tp.close()
    return forms_n, kernels_n, launched


# Forms / kernels no case of this tier can catch next to a padded tensor or a caller buffer, and why.
_HALF_MAP = "B*(H/2)*(W/2)*C*esz with (H/2)*(W/2) % 256 == 0"
TRAIN_FORM_EXCEPTIONS = {
    # the stem's z and G are B x H/2 x W/2 x C with H % 32 == W % 32 == 0 (fd_train_plan_create): (H/2)(W/2) is a multiple of 256; it has no producer
    "stem": _HALF_MAP,
    # the head's z and G are B x H/2 x W/2 x 1 floats (the prediction is upsampled by fd_head_apply_f32 on its way to y) and its producer's tensors
    # B x H/2 x W/2 x C: multiples of 256 x 4 resp. 256 x 2 bytes
    "head": _HALF_MAP,
}
TRAIN_KERNEL_EXCEPTIONS = {
    "fd_stem_train": _HALF_MAP, "fd_stem_wgrad": _HALF_MAP, "fd_stem_wgrad_rows": _HALF_MAP,              # the stem's kernels: "stem" above
    "fd_head_train": _HALF_MAP, "fd_head_bwd_reduce_f32": _HALF_MAP, "fd_head_bwd": _HALF_MAP,            # the head's kernels: "head" above
    # writes the 16-bit operand copies of the pointwise weights (wt, wtt) before the first unit: regions fd_train_layer_tensor does not expose, no caller
    # buffer.  (Their padded rows and columns are what the stale-contents comparison of every 16-bit train case is about.)
    "fd_pack_train_w_h16": "writes private operand copies only",
}


def check_train_coverage(kind):
    t0 = time.time()
    forms_n, kernels_n, launched = train_census(kind)
    forms.note(kind, "family_coverage", "train_forms", t0, **forms_n)
    if kind == "hip":
        forms.note(kind, "family_coverage", "train_kernels", t0, **kernels_n)
        forms.note(kind, "family_coverage", "train_kernel_launches", t0, **launched)
    missing = [f for f in TRAIN_FORMS if not forms_n[f] and f not in TRAIN_FORM_EXCEPTIONS]
    assert not missing, "no train case of the table catches these forms on a unit with a padded tensor: %s" % missing
    assert all(forms_n[f] == 0 for f in TRAIN_FORM_EXCEPTIONS), "an exception of the table is no exception: %s" % forms_n
    if kind == "hip":
        assert all(launched.values()), "train kernels no case of the table launches: %s" % [k for k in TRAIN_KERNELS if not launched[k]]
        missing = [k for k in TRAIN_KERNELS if not kernels_n[k] and k not in TRAIN_KERNEL_EXCEPTIONS]
        assert not missing, "no train case of the table launches these kernels next to a padded tensor or on a caller buffer: %s" % missing
        assert all(kernels_n[k] == 0 for k in TRAIN_KERNEL_EXCEPTIONS), "an exception of the table is no exception: %s" % kernels_n


# ---- caller pointers --------------------------------------------------------------------------------------------------------------------

def _rc(lib, rc, want_text):
    msg = lib.fd_last_error().decode()
    assert rc == -1 and want_text in msg, (rc, msg)          # FD_ERR_INVALID


def check_pointer_contract_inference(kind):
    """include/fastdepth_hip.h: fd_forward refuses an x that is not 16-byte aligned and a y that is not 8-byte aligned (a view 4 bytes past a 16-byte boundary)
    with FD_ERR_INVALID before anything is launched: y and the workspace guards stay as they were."""
    t0 = time.time()
    m = model_of("tiny").eval()
    x = input_of((1, 32, 32)).to(forms.device_of(kind))
    cp = harness.CPlan(kind, m, x, keep=False, fill=0xA5, guard=GUARD)
    try:
        want = harness.bits_of(cp.forward(x, guarded=True))
        ws = cp.ws.clone()
        for arg in ("x", "y"):
            io = harness.Arena(cp.dev, [("x", torch.float32, tuple(x.shape)), ("y", torch.float32, (1, 1, 32, 32))], shift={arg: 4})
            io.view("x").copy_(x)
            assert io.ptr(arg) % 16 == 4
            snap = io.raw.clone()
            _rc(cp.lib, cp.lib.fd_forward(cp.h, io.ptr("x"), io.ptr("y"), cp.stream), "%s must be" % arg)
            if x.is_cuda:
                torch.cuda.synchronize()
            assert torch.equal(io.raw, snap) and torch.equal(cp.ws, ws), "a refused call wrote something"
            ms = (ctypes.c_float * len(cp.layers))()
            _rc(cp.lib, cp.lib.fd_forward_timed(cp.h, io.ptr("x"), io.ptr("y"), cp.stream, ms, len(cp.layers)), "%s must be" % arg)
            if x.is_cuda:
                torch.cuda.synchronize()
            assert torch.equal(io.raw, snap) and torch.equal(cp.ws, ws), "a refused call wrote something"
        # accepted: y 8 bytes past a 16-byte boundary (the head kernels store y as 8-byte pixel pairs: fd_f32x2)
        y8 = harness.bits_of(cp.forward(x, guarded=True, shift={"y": 8}))
        assert cp.io.ptr("y") % 16 == 8 and cp.bad_guards() == 0
        again = harness.bits_of(cp.forward(x, guarded=True))
        assert cp.bad_guards() == 0
    finally:
        cp.close()
    # accepted: every parameter 4 bytes past a 16-byte boundary in fd_plan_pack_weights (fd_pack_fold reads them element by element)
    cp = harness.CPlan(kind, m, x, keep=False, fill=0xA5, guard=GUARD, param_shift=4)
    try:
        assert cp.pa.ptr((0, "conv_weight")) % 16 == 4 and cp.pa.ptr((len(cp.layers) - 1, "bn_var")) % 16 == 4
        p4 = harness.bits_of(cp.forward(x, guarded=True))
        assert cp.bad_guards() == 0
    finally:
        cp.close()
    forms.note(kind, "pointer_contract", "inference", t0, refused="fd_forward:x+4,y+4;fd_forward_timed:x+4,y+4", accepted="y+8,parameters+4",
               bytes_that_differ=int((y8 != want).sum() + (p4 != want).sum() + (again != want).sum()))
    assert np.array_equal(again, want) and np.array_equal(y8, want) and np.array_equal(p4, want)


def check_pointer_contract_train(kind):
    """fd_train_forward refuses a misaligned x, y and conv_weight, fd_train_backward a misaligned conv_weight (FD_ERR_INVALID, nothing launched).  dy, every
    gradient tensor, the BatchNorm vectors, the running statistics (4 bytes) and num_batches_tracked (8 bytes) need their natural alignment only -- the kernels
    touch them element by element: a step with all of them 4 (8) bytes past a 16-byte boundary is bit-equal to the aligned step, guards untouched."""
    t0 = time.time()
    m = model_of("tiny").train()
    shape = (2, 32, 32)
    x, target = _train_inputs(shape)
    want, _ = _train_run(kind, m, x, target, torch.float32, 0, False, 0xA5, "guarded")
    n = len(harness.layers_of(m))
    dev = forms.device_of(kind)
    refused = []
    for arg in ("x", "y", "conv_weight"):
        key = (n // 2, "conv_weight") if arg == "conv_weight" else arg
        tp = harness.CTrainPlan(kind, m, x.to(dev), dtype=torch.float32, fill=0xA5, guard=GUARD, layout="guarded", shift={key: 4})
        try:
            ws = tp.ws.clone()
            io = harness.Arena(dev, [("x", torch.float32, tuple(x.shape)), ("y", torch.float32, (shape[0], 1, shape[1], shape[2]))], shift=tp.shift)
            io.view("x").copy_(x.to(dev))
            snap = io.raw.clone()
            _rc(tp.lib, tp.lib.fd_train_forward(tp.h, tp.params, tp.n, tp.eps, tp.momentum, io.ptr("x"), io.ptr("y"), tp.stream), "%s must be" % arg)
            if dev.type == "cuda":
                torch.cuda.synchronize()
            assert torch.equal(io.raw, snap) and torch.equal(tp.ws, ws) and tp.bad_guards() == 0, "a refused call wrote something"
            refused.append("forward:%s+4" % arg)
        finally:
            tp.close()
    # fd_train_backward: an aligned forward first, then the parameter table with one conv_weight moved
    tp = harness.CTrainPlan(kind, m, x.to(dev), dtype=torch.float32, fill=0xA5, guard=GUARD, layout="guarded")
    try:
        y = tp.forward(x.to(dev))
        dy = (torch.sign(y.cpu() - target) / y.numel()).to(dev)
        grads = (capi.LayerGrads * tp.n)()
        gbuf = torch.zeros(sum(t.numel() for d in tp.tensors for t in d.values()) + 64, device=dev)
        for g in grads:
            g.conv_weight = g.bn_weight = g.bn_bias = gbuf.data_ptr()          # (never written: the call is refused)
        good = tp.params[n // 2].conv_weight
        tp.params[n // 2].conv_weight = good + 4
        _rc(tp.lib, tp.lib.fd_train_backward(tp.h, tp.params, grads, tp.n, dy.data_ptr(), tp.stream), "conv_weight must be")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert not bool(gbuf.any()), "a refused call wrote something"
        tp.params[n // 2].conv_weight = good
        refused.append("backward:conv_weight+4")
    finally:
        tp.close()
    # accepted: everything the kernels touch element by element, 4 (num_batches_tracked: 8) bytes past a 16-byte boundary
    kinds = ("conv_weight", "bn_weight", "bn_bias", "bn_mean", "bn_var")
    shift = {(i, k): 4 for i in range(n) for k in kinds if k != "conv_weight"}
    shift.update({"dy": 4, "nbt": 8})
    tp = harness.CTrainPlan(kind, m, x.to(dev), dtype=torch.float32, fill=0xA5, guard=GUARD, layout="guarded", shift=shift)
    try:
        # (the gradient arena is keyed like the parameters: every gradient view, conv_weight's included, moves by 4 bytes)
        tp.shift = dict(shift)
        tp.shift.update({(i, "conv_weight"): 4 for i in range(n)})
        got, fig = _train_step(tp, x, target, False, 0xA5)
        assert tp.dio.ptr("dy") % 16 == 4 and tp.ga.ptr((0, "conv_weight")) % 16 == 4 and tp.pa.ptr((1, "bn_mean")) % 16 == 4 and tp.pa.ptr("nbt") % 16 == 8
    finally:
        tp.close()
    d = _first_train_difference(want, got, harness.layers_of(m))
    forms.note(kind, "pointer_contract", "train", t0, refused=",".join(refused), accepted="dy+4,gradients+4,bn_vectors+4,running_statistics+4,num_batches_tracked+8", differs=d or "none",
               guards_bad=fig["guards_bad"])
    assert d is None and fig["guards_bad"] == 0 and not fig["inputs_changed"], (d, fig)
