"""The kernel-form matrix of the small-shape tiers: models, case tables, tolerances and one `check_*(kind, ...)` function per check.
TEST INFRASTRUCTURE ONLY: shared by the CPU tier (tests/test_emu_forward.py, tests/test_emu_train.py: kind = "emu", the kernels compiled
with -DFD_EMU on CPU tensors) and the GPU tier (tests/test_gpu_forms.py: kind = "hip", the product library on an MI355X).  Same models,
seeds, shapes, tolerances and assertions in both; the device follows from `kind`."""
import ctypes
import functools
import time
import zlib

import torch

import harness
from fastdepth_hip import capi
from oracle import inputs

TOL = 1e-3    # north-star tolerance: 1e-3 relative, fp32


def device_of(kind):
    return torch.device("cpu" if kind == "emu" else "cuda")


def note(kind, check, case, t0, **figures):
    """One line per executed case (pytest -s / -rA shows it; tools/README.md: how profiles/gpu_forms.txt is made from these lines)."""
    print("FORMS %s %s[%s] %s wall=%.2fs" % (kind, check, case, " ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in figures.items()), time.time() - t0))


def small_model(enc, dec, seed):
    models = inputs.product_models()
    torch.manual_seed(seed)
    m = models.MobileNetSkipAdd((64, 64), pretrained=False, channels=(enc, dec))
    return harness.randomize_bn(m, seed + 1)


TINY = ((8, 16, 24, 24, 32, 32, 40, 40, 40, 40, 40, 40, 48, 48), (40, 32, 24, 16, 8, 1))
RAGGED = ((16, 56, 88, 120, 144, 72, 104, 40, 72, 88, 96, 128, 80, 112), (200, 72, 120, 56, 16, 1))   # multiples of 8, like the pruned plan
G16 = ((32, 32, 64, 64, 96, 96, 128, 128, 128, 128, 128, 128, 160, 160), (128, 96, 64, 32, 32, 1))    # every pointwise reduction a multiple of 32 (fd_pw_gemm16_f32 train mode); 96 / 160 outputs: a ragged last 64-column tile
UNITS = ((32, 64, 128, 128, 256, 256, 40, 40, 40, 40, 40, 40, 48, 48), (40, 256, 128, 64, 32, 1))   # the large-map units at full width
WIDE = ((16, 32, 64, 64, 128, 128, 40, 40, 40, 40, 40, 40, 48, 16), (200, 128, 64, 32, 16, 1))   # 64-channel depthwise blocks (cb = 64), a padded pruned width, a 16-channel block

# TINY with ONE wide stage on the 1/4-resolution map (conv2.3 -> conv3.0 -> conv3.3: 264 channels, not a skip source): at 2 x 160 x 224 the backward-data GEMM of
# conv3.3 has M = 4480, K = 264, i.e. ceil(M / 64) x ceil(K / 128) = 70 x 3 = 210 >= 200 workgroups -- the smallest setting of this matrix's shapes at which the
# paired 16-bit pointwise backward takes its 64 x 128 tiles under FD_TUNE_PW_PAIR_TN2 (launch_pw_bwd_h16, csrc/fd_train_bwd_impl.h); the last k tile is ragged (8 channels)
TN2 = ((8, 16, 264, 24, 32, 32, 40, 40, 40, 40, 40, 40, 48, 48), (40, 32, 24, 16, 8, 1))

F = capi

# ---- inference --------------------------------------------------------------------------------------------------------------------------

FORWARD_CASES = [("tiny", TINY, 2, 64), ("ragged", RAGGED, 1, 64), ("tiny_rect", TINY, 1, (32, 96))]


def check_forward_matches_oracle(kind, name, plan, b, hw):
    t0 = time.time()
    h, w = (hw, hw) if isinstance(hw, int) else hw
    m = small_model(plan[0], plan[1], seed=zlib.crc32(name.encode()) % 1000)      # (a fixed seed per case name: both tiers check the same model)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(b, 3, h, w, generator=g)
    err, per_layer, info = harness.compare_with_oracle(kind, m, x, device_of(kind))
    note(kind, "forward_matches_oracle", name, t0, output=err, worst_layer=max(per_layer), tol=TOL)
    bad = [(i, e, info[i]) for i, e in enumerate(per_layer) if not e < TOL]
    assert not bad, "layers out of tolerance: %s" % bad
    assert err < TOL


GEMM16_CASES = [("ragged", RAGGED, 2, (32, 96)), ("tiny", TINY, 2, 64)]


def check_gemm16_matches_oracle(kind, name, plan, b, hw):
    """fd_pw_gemm16_f32 (16x16x4 MFMA, k-split wave pairs, leader/follower LDS-DMA, LDS-transposed epilogue) forced onto every
    pointwise layer: the batch / image sizes make M = 1536, 384, 96, 24, 6 (ragged) resp. 2048 ... 8 (tiny), i.e. all three row-tile
    counts (13, 7, 4), strides below the full tile, ragged M, ragged N (not a multiple of 64) and ragged K (not a multiple of 32)."""
    t0 = time.time()
    h, w = (hw, hw) if isinstance(hw, int) else hw
    m = small_model(plan[0], plan[1], seed=21)
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(8))
    err, per_layer, info = harness.compare_with_oracle(kind, m, x, device_of(kind), flags=F.FD_TUNE_FORCE_GEMM16)
    note(kind, "gemm16_matches_oracle", name, t0, output=err, worst_layer=max(per_layer), tol=TOL)
    used = [s for s in info if s.startswith("pw_gemm16")]
    assert len(used) == 18, info
    if name == "ragged":
        assert {s.split("TM=")[1].split(":")[0] for s in used} == {"13", "7", "4"}, used
    if name == "tiny":
        # 64 x 64 frames: from 4 x 4 down a workgroup holds whole frames, so the depthwise consumers run in the GEMM epilogues -- all four
        # variants: 3x3 stride 1, 3x3 stride 2, 5x5, 5x5 on the nearest-x2 upsampling (each checked layer-wise against the oracle above)
        fused = [s for s in info if "evaluated in the epilogue" in s]
        assert {s.split("(dw ")[1].split(" evaluated")[0] for s in fused} >= {"k3 s1", "k3 s2", "k5 s1", "k5 s1 on up2"}, fused
    bad = [(i, e, info[i]) for i, e in enumerate(per_layer) if not e < TOL]
    assert not bad and err < TOL, bad


DWPW_CASES = [(2, (64, 64)), (1, (96, 160)), (9, (32, 32))]


@functools.lru_cache(maxsize=None)
def _units_case(b, hw):
    """(module, x, oracle output, oracle taps) of one fd_dwpw_f32 case: computed once, shared by both tiers' cases, never modified."""
    from oracle import oracle
    m = small_model(UNITS[0], UNITS[1], seed=31).eval()
    x = torch.rand(b, 3, *hw, generator=torch.Generator().manual_seed(9))
    y_ref, taps_ref = oracle.forward(m.state_dict(), x.numpy(), taps=True)
    return m, x, y_ref, taps_ref


def check_dwpw_units_match_oracle(kind, b, hw):
    """fd_dwpw_f32 (depthwise + pointwise unit of a large map as ONE persistent, wave-specialised kernel: producer waves stage patch
    chunks and run the depthwise taps into the GEMM's A tile, consumer waves run the 32x32x2 MFMAs over all output channels) forced
    onto every eligible pair: conv1 / conv3 (3x3 stride 1), conv2 (3x3 stride 2, 64-pixel tiles), decode_conv4 / 5 (5x5 on up2(low) +
    skip); 1..4 channel chunks, several tiles per workgroup at batch 2, ragged tiles (96 x 160 input: 48 x 80, 24 x 40 maps), checked
    layer by layer against the oracle."""
    t0 = time.time()
    dev = device_of(kind)
    m, x, y_ref, taps_ref = _units_case(b, hw)
    xd = x.to(dev)
    cp = harness.CPlan(kind, m, xd, keep=True, flags=F.FD_TUNE_FORCE_UNIT_FUSION)
    try:
        info = cp.info()
        y = cp.forward(xd).cpu().numpy()
        units = [i for i, s in enumerate(info) if s.startswith("dwpw<")]
        assert len(units) == 5, info
        assert {info[i].split("<")[1].split(" +")[0] for i in units} == {"dw k3 s1 mode0", "dw k3 s2 mode0", "dw k5 s1 mode2"}, info
        worst = 0.0
        for i in range(len(taps_ref) - 1):
            if info[i].startswith("(fused into"):
                continue
            e = harness.rel_err(cp.tap(i).numpy(), taps_ref[i])
            worst = max(worst, e)
            assert e < TOL, (i, e, info[i])
        e_forced = harness.rel_err(y, y_ref)
        assert e_forced < TOL
    finally:
        cp.close()
    # the default plan (no force flag, no kept activations) selects the kernel only where it was measured to pay: units with <= 64 depthwise
    # channels on maps of >= 28 x 28 pixels (conv1, conv2, decode_conv5)
    cp = harness.CPlan(kind, m, xd, keep=False)
    try:
        sel = [s for s in cp.info() if s.startswith("dwpw<")]
        if hw != (32, 32):
            # decode_conv5's unit also evaluates the network head (32 -> 1 pointwise, written 2x2) on its accumulators
            assert sum("head on the accumulators" in s for s in sel) == 1 and any(s.startswith("(pointwise head evaluated") for s in cp.info()), cp.info()
        y2 = cp.forward(xd).cpu().numpy()
    finally:
        cp.close()
    e_default = harness.rel_err(y2, y_ref)
    note(kind, "dwpw_units_match_oracle", "%dx%dx%d" % (b, hw[0], hw[1]), t0, worst_layer=worst, output_forced=e_forced, output_default=e_default, tol=TOL)
    assert len(sel) == {(64, 64): 2, (96, 160): 3, (32, 32): 0}[hw], sel     # (batch 9: images dealt to XCDs, a ragged last group)
    assert e_default < TOL


H16_FORWARD_DTYPES = [(torch.float16, 5e-3), (torch.bfloat16, 4e-2)]
H16_FORWARD_MODELS = [("tiny", TINY), ("ragged", RAGGED)]


def check_16bit_forward_matches_oracle(kind, name, plan, dtype, tol):
    """16-bit activation / pointwise-weight storage (fp32 accumulate): bounded drift against the fp32 oracle.  The reference's
    own drift when run in fp16 / bf16 is 9e-4 / 7.6e-3 max-rel on the NYU sample; the tiny random nets used
    here are less forgiving, hence the looser bounds."""
    t0 = time.time()
    m = small_model(plan[0], plan[1], seed=21)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(6))
    err, per_layer, info = harness.compare_with_oracle(kind, m, x, device_of(kind), dtype=dtype)
    note(kind, "16bit_forward_matches_oracle", "%s-%s" % (name, str(dtype).split(".")[-1]), t0, output=err, tol=tol, worst_layer=max(per_layer), layer_tol=4 * tol)
    assert err < tol, (err, max(per_layer))
    assert max(per_layer) < 4 * tol, [(i, e, info[i]) for i, e in enumerate(per_layer) if e >= 4 * tol]


def _unit64(t, conv, bn, act):
    import torch.nn.functional as Fn
    t = Fn.conv2d(t.double(), conv.weight.double(), None, conv.stride, conv.padding, 1, conv.groups)
    t = Fn.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
    return t.clamp(0, 6) if isinstance(act, torch.nn.ReLU6) else t.clamp(min=0)


def check_no_skip_sibling_forward(kind):
    """Row f-3: the no-skip `MobileNet('nnconv5dw')` runs on the same kernels (plan walk `mobilenet.*` / `decoder.*`, nearest x2
    folded into the next unit's read, skip = -1).  Full widths, 32x32 input, against a torch-functional restatement of the
    reference's forward (models.py:244-270, 455-458) built from the product module's own tensors."""
    import torch.nn.functional as Fn
    t0 = time.time()
    models = inputs.product_models()
    torch.manual_seed(21)
    m = harness.randomize_bn(models.MobileNet("nnconv5dw", (32, 32), pretrained=False), 22).eval()
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(23))

    def unit(t, seq):
        mods = list(seq)
        for i in range(0, len(mods), 3):
            t = _unit64(t, *mods[i:i + 3])
        return t

    with torch.no_grad():
        t = x
        for blk in m.mobilenet:
            t = unit(t, blk)
        for j in range(1, 6):
            blk = getattr(m.decoder, "conv%d" % j)
            t = unit(unit(t, blk[0]), blk[1])
            t = Fn.interpolate(t, scale_factor=2, mode="nearest")
        ref = unit(t, m.decoder.conv6)
    xd = x.to(device_of(kind))
    plan = harness.CPlan(kind, m, xd, keep=False)
    try:
        y = plan.forward(xd).cpu()
    finally:
        plan.close()
    e = harness.rel_err(y.numpy(), ref.numpy())
    note(kind, "no_skip_sibling_forward", "32x32", t0, output=e, tol=TOL)
    assert e < TOL


def check_skip_concat_sibling_forward(kind):
    """Row f-3: `MobileNetSkipConcat` -- the depthwise kernel reads cat(up2(x), skip) as two channel ranges of two tensors
    (fd_layer_desc.concat, MODE 3).  Full widths, 32x32 input, against a torch-functional restatement of the reference's
    forward (models.py:786-813) built from the product module's own tensors."""
    import torch.nn.functional as Fn
    t0 = time.time()
    models = inputs.product_models()
    torch.manual_seed(31)
    m = harness.randomize_bn(models.MobileNetSkipConcat((32, 32), pretrained=False), 32).eval()
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(33))

    def unit(t, seq):
        mods = []
        for c in seq:
            mods += list(c) if isinstance(c, torch.nn.Sequential) else [c]
        for i in range(0, len(mods), 3):
            t = _unit64(t, *mods[i:i + 3])
        return t

    with torch.no_grad():
        t, skips = x, {}
        for i in range(14):
            t = unit(t, getattr(m, "conv%d" % i))
            if i in (1, 3, 5):
                skips[i] = t
        for j in range(1, 6):
            t = unit(t, getattr(m, "decode_conv%d" % j))
            t = Fn.interpolate(t, scale_factor=2, mode="nearest")
            if j in (2, 3, 4):
                t = torch.cat((t, skips[{2: 5, 3: 3, 4: 1}[j]]), 1)
        ref = unit(t, m.decode_conv6)
    xd = x.to(device_of(kind))
    plan = harness.CPlan(kind, m, xd, keep=False)
    try:
        y = plan.forward(xd).cpu()
    finally:
        plan.close()
    e = harness.rel_err(y.numpy(), ref.numpy())
    note(kind, "skip_concat_sibling_forward", "32x32", t0, output=e, tol=TOL)
    assert e < TOL


ULP_DTYPES = [(torch.float16, 2.0 ** -10), (torch.bfloat16, 2.0 ** -7)]
H16_GEMM16_CASES = [("tiny", TINY, 2, (64, 64), F.FD_TUNE_FORCE_EPILOGUE_FUSION), ("tiny5", TINY, 5, (64, 64), F.FD_TUNE_FORCE_EPILOGUE_FUSION),
                    ("ragged", RAGGED, 2, (64, 64), F.FD_TUNE_FORCE_EPILOGUE_FUSION),
                    ("ragged_forced", RAGGED, 2, (32, 96), F.FD_TUNE_FORCE_GEMM16),
                    ("tiny_forced", TINY, 3, (64, 64), F.FD_TUNE_FORCE_GEMM16)]


def check_16bit_gemm16_and_fused_epilogues(kind, name, plan, b, hw, flags, dtype, ulp):
    """fd_pw_gemm16_h16 (16x16x32 MFMA, whole frames per workgroup, depthwise consumer in the epilogue) against the first-generation 16-bit
    kernels (fd_pw_gemm_h16 + separate depthwise launches) on the same plan: both round the pointwise output to the storage type before the
    depthwise layer reads it, so every stored tensor agrees to the last bit or two of the storage type (the k-halves are summed in a different
    order).  FORCE_EPILOGUE_FUSION picks the kernel wherever a depthwise consumer fuses behind it (maps of <= 208 pixels; product plans: only where
    it was measured to pay); FORCE_GEMM16 puts it on every pointwise layer (ragged M / N / K, strides that are not whole frames: no fusion there)."""
    t0 = time.time()
    m = small_model(plan[0], plan[1], seed=21).eval()
    x = torch.rand(b, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(8)).to(device_of(kind))
    new = harness.CPlan(kind, m, x, dtype=dtype, flags=flags)
    old = None
    try:
        old = harness.CPlan(kind, m, x, dtype=dtype, flags=F.FD_PLAN_NO_GEMM16 | F.FD_PLAN_NO_EPILOGUE_FUSION | F.FD_PLAN_NO_ROWS8)   # (also: 4- instead of 8-channel 3x3 depthwise kernel)
        y_new, y_old = new.forward(x).cpu(), old.forward(x).cpu()
        info = new.info()
        used = [s for s in info if s.startswith("pw_gemm16")]
        fused = [s for s in info if "evaluated in the epilogue" in s]
        assert not any(s.startswith("pw_gemm16") for s in old.info())
        if flags == F.FD_TUNE_FORCE_GEMM16:
            assert len(used) == 18, info
        else:
            assert len(used) >= 6 and len(fused) == len(used), info           # picked exactly where a consumer fuses
            if name.startswith("tiny"):
                assert {s.split("(dw ")[1].split(" evaluated")[0] for s in fused} >= {"k3 s1", "k3 s2", "k5 s1", "k5 s1 on up2"}, fused
        n = len(new.layers)
        worst = 0.0
        for i in range(n - 1):
            a, r = new.tap(i).double(), old.tap(i).double()
            d = float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)
            worst = max(worst, d)
            assert float((a - r).abs().max()) <= 2.5 * ulp * max(float(r.abs().max()), 1e-30), (i, info[i])
        e = harness.rel_err(y_new.numpy(), y_old.numpy())
        note(kind, "16bit_gemm16_and_fused_epilogues", "%s-%s" % (name, str(dtype).split(".")[-1]), t0, worst_layer=worst, layer_tol=2.5 * ulp, output=e, tol=4 * ulp)
        assert e < 4 * ulp
    finally:
        new.close()
        if old is not None:
            old.close()


H16_DTYPES = [torch.float16, torch.bfloat16]


def check_16bit_head_on_the_last_gemm(kind, name, plan, dtype):
    """16-bit product plans evaluate the network head (decode_conv6: Cout -> 1 pointwise + ReLU, nearest x2) on the output tile of decode_conv5.1's
    GEMM (fd_pw_gemm_head_h16: that layer's tensor is neither written nor re-read).  Same arithmetic as the separate head kernel on the stored
    tensor (the tile is rounded to the storage type first), different summation order: the two plans agree to fp32 rounding."""
    t0 = time.time()
    m = small_model(plan[0], plan[1], seed=33).eval()
    x = torch.rand(3, 3, 64, 96, generator=torch.Generator().manual_seed(12)).to(device_of(kind))
    fused = harness.CPlan(kind, m, x, keep=False, dtype=dtype)
    plain = None
    try:
        plain = harness.CPlan(kind, m, x, keep=False, dtype=dtype, flags=F.FD_PLAN_NO_EPILOGUE_FUSION)
        info = fused.info()
        assert any("head on its output tile" in s for s in info) and any("pointwise head evaluated" in s for s in info), info
        assert not any("head on its output tile" in s for s in plain.info())
        ya, yb = fused.forward(x).cpu(), plain.forward(x).cpu()
        e = harness.rel_err(ya.numpy(), yb.numpy())
        note(kind, "16bit_head_on_the_last_gemm", "%s-%s" % (name, str(dtype).split(".")[-1]), t0, output=e, tol=2e-6)
        assert ya.shape == (3, 1, 64, 96) and e < 2e-6
    finally:
        fused.close()
        if plain is not None:
            plain.close()


DW_H8_CASES = [(2, (64, 64)), (1, (64, 96))]


def check_16bit_depthwise_8_channels_per_work_item(kind, b, hw, dtype, ulp):
    """16-bit plans run the LDS-tiled depthwise layers (the decoder's 5x5 units: plain, on up2, on up2 + skip) with storage-typed LDS patches and
    8 channels (16 bytes) per work-item (fd_dwconv<T, ..., 8>) where that was measured to pay (the large maps) or, as here, under FD_TUNE_FORCE_DW_H8 wherever
    eligible; FD_TUNE_NO_DW_H8 keeps the fp32-patch / 4-channel form everywhere.  Plain and upsampled inputs
    are copied into LDS bit for bit and the taps accumulate in fp32 in the same order, so those layers agree exactly; the up2(low) + skip sum is
    rounded to the storage type on its way into LDS (the 4-channel form keeps it in fp32): one extra rounding of the conv input."""
    t0 = time.time()
    m = small_model(WIDE[0], WIDE[1], seed=44).eval()
    x = torch.rand(b, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(13)).to(device_of(kind))
    # (FD_TUNE_NO_DW5_ROWS: since round 6 the up2 + skip units of a product plan run on fd_dw5_rows -- test below; this test keeps the LDS-tiled form on them)
    new = harness.CPlan(kind, m, x, dtype=dtype, flags=F.FD_PLAN_NO_EPILOGUE_FUSION | F.FD_TUNE_FORCE_DW_H8 | F.FD_TUNE_NO_DW5_ROWS)
    old = None
    try:
        old = harness.CPlan(kind, m, x, dtype=dtype, flags=F.FD_PLAN_NO_EPILOGUE_FUSION | F.FD_TUNE_NO_DW_H8 | F.FD_TUNE_NO_DW5_ROWS)
        info = new.info()
        h8 = [i for i, s in enumerate(info) if s.startswith("dwconv<") and "8 channels per work-item" in s]
        assert len(h8) == 5 and {info[i].split("tile ")[1].split(" ")[0].split("x")[2] for i in h8} >= {"64", "32", "16"}, info
        assert not any("8 channels per work-item" in s for s in old.info())
        y_new, y_old = new.forward(x).cpu(), old.forward(x).cpu()
        prev_exact = True
        worst = worst_exact = 0.0
        for i in range(len(new.layers) - 1):
            a, r = new.tap(i).double(), old.tap(i).double()
            d = float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)
            worst = max(worst, d)
            if i in h8 and prev_exact and "mode2" not in info[i]:
                worst_exact = max(worst_exact, d)
                assert d == 0.0, (i, info[i], d)                  # same inputs, bit-for-bit staging, same accumulation order
            assert d <= 3.0 * ulp, (i, info[i], d)
            prev_exact = prev_exact and d == 0.0
        e = harness.rel_err(y_new.numpy(), y_old.numpy())
        note(kind, "16bit_depthwise_8_channels_per_work_item", "%dx%dx%d-%s" % (b, hw[0], hw[1], str(dtype).split(".")[-1]), t0, bit_equal_layers=worst_exact, bit_equal_tol=0.0,
             worst_layer=worst, layer_tol=3.0 * ulp, output=e, tol=6 * ulp)
        assert e < 6 * ulp
    finally:
        new.close()
        if old is not None:
            old.close()


DW5_ROWS_CASES = [(2, (64, 64)), (1, (64, 96)), (1, (32, 32))]


def check_16bit_dw5_rows_pixel_pair_kernel(kind, b, hw, dtype, ulp):
    """Round 6: the 5x5 units on up2(low) + skip (decode_conv3 / 4 / 5) of a 16-bit plan run on fd_dw5_rows (fd_kernels_dw5p.h): independent waves walk
    down bands of rows with the input window as PIXEL PAIRS and the taps as 16-bit pairs in registers, v_dot2 accumulation in fp32, raw-buffer access
    with the horizontal padding done by the range check.  Against the LDS-tiled fp32-patch form (FD_TUNE_NO_DW5_ROWS | FD_TUNE_NO_DW_H8) on the SAME stored
    inputs it differs by the rounding of the up2 + skip sum and of the 25 folded taps to the storage type: a few units in the last place of the layer's
    range.  Shapes: 64-channel blocks, a ragged pruned width (200 = 4 x 56 - 24), 16- and 32-channel units (half-empty waves), bands with a ragged last
    band (H = 8 ... 32), the 128-channel wave form (3 strips per row at 64 x 96: odd)."""
    t0 = time.time()
    m = small_model(WIDE[0], WIDE[1], seed=45).eval()
    x = torch.rand(b, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(14)).to(device_of(kind))
    new = harness.CPlan(kind, m, x, dtype=dtype, flags=F.FD_PLAN_NO_EPILOGUE_FUSION)
    old = None
    try:
        old = harness.CPlan(kind, m, x, dtype=dtype, flags=F.FD_PLAN_NO_EPILOGUE_FUSION | F.FD_TUNE_NO_DW5_ROWS | F.FD_TUNE_NO_DW_H8)
        info = new.info()
        rows = [i for i, s in enumerate(info) if s.startswith("dw5_rows<")]
        assert len(rows) == 3 and all("mode2" in info[i] for i in rows), info
        assert not any(s.startswith("dw5_rows<") for s in old.info())
        if hw == (64, 96):
            assert any("64 channel lanes per strip" in info[i] for i in rows), info
        y_new, y_old = new.forward(x).cpu(), old.forward(x).cpu()
        worst = 0.0
        for i in rows:
            # the unit on ITS OWN stored inputs: re-run the reference form's layer i on the new plan's inputs is not possible through the C ABI, so compare
            # the taps of both plans layer by layer -- the layers before the first dw5_rows unit are bit-identical, later ones inherit the earlier difference
            a, r = new.tap(i).double(), old.tap(i).double()
            d = float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)
            worst = max(worst, d)
            assert d <= 6.0 * ulp, (i, info[i], d)
        first = rows[0]
        before = max(float((new.tap(i).double() - old.tap(i).double()).abs().max()) for i in range(first))
        e = harness.rel_err(y_new.numpy(), y_old.numpy())
        note(kind, "16bit_dw5_rows_pixel_pair_kernel", "%dx%dx%d-%s" % (b, hw[0], hw[1], str(dtype).split(".")[-1]), t0, layers_before_first_unit=before, bit_equal_tol=0.0,
             worst_unit=worst, unit_tol=6.0 * ulp, output=e, tol=8 * ulp)
        for i in range(first):
            assert float((new.tap(i).double() - old.tap(i).double()).abs().max()) == 0.0, (i, info[i])
        assert e < 8 * ulp
    finally:
        new.close()
        if old is not None:
            old.close()


# ---- train step -------------------------------------------------------------------------------------------------------------------------

TRAIN_E2E_CASES = [("tiny", TINY, 2), ("tiny_sat6", TINY, 2)]     # (the ragged widths run through the layer-local check below)


def check_train_forward_backward(kind, name, plan, b):
    t0 = time.time()
    m = small_model(plan[0], plan[1], seed=3)
    if name.endswith("sat6"):
        harness.saturate_encoder(m)              # encoder gamma x 4: the clamp-at-6 side of the ReLU6 masks
    g = torch.Generator().manual_seed(9)
    x = torch.rand(b, 3, 64, 64, generator=g)
    target = 2.0 + torch.rand(b, 1, 64, 64, generator=g)
    rep = harness.train_parity_report(kind, m, x, target, device_of(kind), kink=1e-3 if name.endswith("sat6") else 1e-4)
    # (sat6: the pre-activations are 4x larger and, at this size, agree with the oracle to ~4e-4 of their scale only -- see below)
    # 64x64 inputs leave 2x2 pixels x batch 2 = 8 samples per channel at the deepest BatchNorms: the train-mode forward is
    # ill-conditioned there (pre-activations agree to ~4e-4 only), and the backward inherits that -> looser bound than on the
    # full-size GPU test
    # (the saturating variant has twice as many kinks per unit: its end-to-end bound is looser still; the sharp statement about the
    # clamp-at-6 mask is the layer-local check below, at 2e-5)
    tol = 1e-2 if name.endswith("sat6") else 5e-3
    floor = 1e-5 * rep["global_norm"]
    worst_grad = max([v[0] / v[1] for v in rep["tensors"].values() if v[0] > floor and v[1] > 0] or [0.0])
    note(kind, "train_forward_backward", name, t0, pred=rep["pred_err"], y=rep["y_err"], running=rep["running"], bad_flips=rep["bad_flips"], worst_grad_above_floor=worst_grad, tol=tol)
    harness.assert_train_parity(rep, tol=tol)
    if name.endswith("sat6"):
        assert harness.LAST_SAT6_FRAC > 0.005, harness.LAST_SAT6_FRAC


LOCAL_TOL = {
    # fp32 plan: every category is fp32 arithmetic on identical inputs
    torch.float32: {"default": 2e-5},
    # bf16 plan: tensors STORED in bf16 carry one rounding (2^-8 relative to the tensor's max is the bound, 2^-9 typical);
    # everything kept in fp32 (tables, running statistics, parameter gradients, prediction) stays at fp32 accuracy
    # (conv_wgrad_lds16: depthwise units whose backward kernels keep bf16 LDS patches -- fp32 result of operands that were rounded from fp32
    # values, against a reference that rounds fp64 values: see harness.local_train_parity)
    torch.bfloat16: {"default": 2e-5, "z": 4e-3, "g_src": 4e-3, "dz": 4e-3, "skip_grad": 4e-3, "conv_wgrad_lds16": 2e-3},
}


def assert_local_parity(rep, dtype):
    tol = LOCAL_TOL[dtype]
    bad = {k: v for k, v in rep.items() if not v[0] <= tol.get(k, tol["default"])}
    assert not bad, "layer-local train parity out of tolerance: %s" % bad
    assert {"z", "bn_table", "running", "bn_grads", "conv_wgrad", "g_src", "skip_grad", "pred", "g_head"} <= set(rep)


def _note_local(kind, check, case, t0, rep, dtype):
    tol = LOCAL_TOL[dtype]
    note(kind, check, case, t0, **{k: "%.3g/%.0e" % (v[0], tol.get(k, tol["default"])) for k, v in sorted(rep.items())})


def flag_names(flags):
    names = [k for k in sorted(dir(capi)) if (k.startswith("FD_TUNE_") or k.startswith("FD_PLAN_NO_")) and k != "FD_TUNE_ALL" and flags & getattr(capi, k)]
    return "|".join(n.replace("FD_TUNE_", "").replace("FD_PLAN_", "") for n in names) or "default"


TRAIN_LOCAL_CASES = [("tiny", TINY, torch.float32, 0), ("tiny", TINY, torch.bfloat16, F.FD_TUNE_WGRAD_TILE_ROWS),
                     ("ragged", RAGGED, torch.bfloat16, 0), ("tiny_wide", TINY, torch.float32, 0),
                     ("tiny_sat6", TINY, torch.float32, 0), ("ragged_sat6", RAGGED, torch.bfloat16, 0),
                     ("tiny", TINY, torch.bfloat16, F.FD_PLAN_NO_BWD_PAIRING),
                     ("tiny", TINY, torch.bfloat16, F.FD_TUNE_DW_BWD_PAIR),
                     ("tiny", TINY, torch.float32, F.FD_TUNE_DW_BWD1),
                     ("tiny", TINY, torch.float32, F.FD_TUNE_DW_PITCH4 | F.FD_TUNE_DW_PITCH8 | F.FD_TUNE_DW_WGRAD_TH4),
                     ("tiny", TINY, torch.float32, F.FD_TUNE_DW_FORCE_ROWS), ("tiny_tall", TINY, torch.bfloat16, F.FD_TUNE_DW_FORCE_ROWS),
                     # fd_lane<T, 8>: bf16 LDS patches, 8 channels per work-item -- paired launch / single-staging kernel, ragged channel counts
                     ("ragged", RAGGED, torch.bfloat16, F.FD_TUNE_FORCE_DW_H8 | F.FD_TUNE_DW_BWD_PAIR),
                     ("tiny", TINY, torch.bfloat16, F.FD_TUNE_FORCE_DW_H8 | F.FD_TUNE_DW_BWD1),
                     # every BatchNorm finalised by its own launch (default at this size: inside the consuming depthwise kernel /
                     # the unit's own first backward kernel, fd_bn_finalize_block / fd_bn_bwd_finalize_block)
                     # fp32 forward pointwise GEMMs on fd_pw_gemm16_f32<..., TRAIN> (TM = 13 / 7 / 4 as the maps shrink; statistics of whole-stride tiles)
                     ("g16", G16, torch.float32, F.FD_TUNE_FORCE_GEMM16), ("g16_sat6", G16, torch.float32, F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_NO_CONSUMER_FINALIZE),
                     ("tiny", TINY, torch.float32, F.FD_TUNE_NO_CONSUMER_FINALIZE),
                     # ... and the depthwise backward launches finalising their own unit too (off by default: measured no faster)
                     ("tiny", TINY, torch.float32, F.FD_TUNE_DW_BWD_FINALIZE), ("ragged", RAGGED, torch.bfloat16, F.FD_TUNE_DW_BWD_FINALIZE | F.FD_TUNE_DW_BWD1),
                     ("ragged", RAGGED, torch.bfloat16, F.FD_TUNE_NO_CONSUMER_FINALIZE),
                     # the tile-geometry and pairing bits of csrc/fd_tuning.h (their effect on the plan: check_train_form_took_effect below)
                     ("tiny", TINY, torch.float32, F.FD_TUNE_DW_TH8), ("ragged", RAGGED, torch.bfloat16, F.FD_TUNE_DW_CB16),
                     ("tiny", TINY, torch.float32, F.FD_TUNE_DW_SMALL_TILES), ("tiny", TINY, torch.bfloat16, F.FD_TUNE_NO_PW_PAIRING),
                     ("ragged", RAGGED, torch.bfloat16, F.FD_TUNE_PW_PAIR_TN2), ("tiny", TINY, torch.bfloat16, F.FD_TUNE_DW_NO_ROWS),
                     # 224 x 32: map heights 112 ... 7 -- 8-row tiles leave a ragged last tile (28 = 3 x 8 + 4, 14 = 8 + 6), in 16-channel blocks
                     ("tiny_tall", TINY, torch.float32, F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16), ("tiny_tall", TINY, torch.bfloat16, F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16),
                     # a bf16 train plan without any row-walking kernel: every depthwise unit LDS-tiled forward and backward, the stem's weight gradient on fd_stem_wgrad
                     ("tiny", TINY, torch.bfloat16, F.FD_TUNE_NO_DW5_ROWS),
                     # the shape at which FD_TUNE_PW_PAIR_TN2 changes a launch: conv3.3 of TN2 (K = 264) on 64 x 128 backward-data tiles, 210 workgroups
                     ("tn2_wide", TN2, torch.bfloat16, F.FD_TUNE_PW_PAIR_TN2)]


def train_local_shape(name):
    # tiny_tall: map heights 112 ... 7 (the 14-row backward-data tiles; H must be a multiple of 32)
    # tiny_wide: > 256 partial rows per reduction (280 for conv1.3 / decode_conv5.1) -> the sliced (last-arriver) path
    return (160, 224) if name in ("tiny_wide", "tn2_wide") else ((224, 32) if name == "tiny_tall" else (64, 64))


def train_local_inputs(name, plan):
    m = small_model(plan[0], plan[1], seed=3)
    if name.endswith("sat6"):
        harness.saturate_encoder(m)
    g = torch.Generator().manual_seed(9)
    h, w = train_local_shape(name)
    x = torch.rand(2, 3, h, w, generator=g)
    target = 2.0 + torch.rand(2, 1, h, w, generator=g)
    return m, x, target


def check_train_step_layer_local(kind, name, plan, dtype, flags):
    """Every unit's forward and backward kernels on their own stored inputs against an fp64 single-unit autograd reference
    (harness.local_train_parity): the rigorous check of the bf16 train plan, whose end-to-end
    comparison is chaotic on a network this small."""
    t0 = time.time()
    m, x, target = train_local_inputs(name, plan)
    # (default plans: a stride-2 depthwise unit's backward is ONE single-staging kernel (fd_dw_bwd1), the other depthwise units' two kernels and a
    # pointwise unit's two GEMMs share a paired launch; FD_TUNE_DW_BWD1 / _PAIR: the single-staging kernel everywhere / nowhere;
    # FD_PLAN_NO_BWD_PAIRING: every kernel on its own)
    rep = harness.local_train_parity(kind, m, x, target, device_of(kind), dtype=dtype, flags=flags)
    _note_local(kind, "train_step_layer_local", "%s-%s-%s" % (name, str(dtype).split(".")[-1], flag_names(flags)), t0, rep, dtype)
    assert_local_parity(rep, dtype)
    info = harness.LAST_LOCAL_INFO
    assert (info["dw_units_with_16bit_lds_patches"] > 0) == bool(flags & F.FD_TUNE_FORCE_DW_H8)
    # round 6: in a bf16 plan the three 5x5 units on up2 + skip run their backward on the row-walking pixel-pair kernel (fd_dw5_bwd_rows) unless a flag
    # asks for one of the LDS-tiled forms
    lds_forms = F.FD_TUNE_DW_BWD1 | F.FD_TUNE_DW_BWD_PAIR | F.FD_TUNE_DW_BWD_FINALIZE | F.FD_TUNE_NO_DW5_ROWS | F.FD_PLAN_NO_BWD_PAIRING
    assert info["dw_units_on_dw5_bwd_rows"] == (3 if dtype == torch.bfloat16 and not flags & lds_forms else 0), info
    # ... and every 3x3 unit of the encoder on fd_dw3_bwd_rows (stride 1: 9 units) / fd_dw3s2_bwd_rows (stride 2: 4 units)
    # (FD_TUNE_DW_FORCE_ROWS keeps the stride-2 units on the older two register-window kernels; FD_TUNE_DW_NO_ROWS puts them on the LDS-tiled
    # single-staging kernel -- dw_bwd_plan tests that bit for the stride-2 forms only, the stride-1 units stay on fd_dw3_bwd_rows)
    on_rows = 0 if dtype != torch.bfloat16 or flags & (lds_forms | F.FD_TUNE_FORCE_DW_H8) else (12 if flags & (F.FD_TUNE_DW_FORCE_ROWS | F.FD_TUNE_DW_NO_ROWS) else 16)
    assert info["dw_units_backward_on_row_kernels"] == on_rows, info
    # ... and the forward of all 13 encoder units on fd_dw3_rows_fwd
    assert info["dw_units_on_dw3_rows_fwd"] == (13 if dtype == torch.bfloat16 and not flags & (F.FD_TUNE_NO_DW5_ROWS | F.FD_TUNE_FORCE_DW_H8 | F.FD_TUNE_DW_FORCE_ROWS | F.FD_TUNE_DW_NO_ROWS) else 0), info
    assert info["dw_units_on_dw5_rows_train"] == (3 if dtype == torch.bfloat16 and not flags & (F.FD_TUNE_NO_DW5_ROWS | F.FD_TUNE_FORCE_DW_H8) else 0), info
    # the forms the flags ask for did run: gemm16 train GEMMs (every pointwise unit but the head), in-kernel finalisations forward / backward
    assert info["pw_units_on_gemm16"] == (18 if name.startswith("g16") else 0)
    assert (info["units_finalised_by_consumer"] > 0) == (not flags & F.FD_TUNE_NO_CONSUMER_FINALIZE)
    if flags & F.FD_TUNE_NO_CONSUMER_FINALIZE:
        assert info["units_finalising_their_own_backward"] == 0
    elif flags & F.FD_TUNE_DW_BWD_FINALIZE:
        assert info["units_finalising_their_own_backward"] >= (12 if dtype == torch.float32 else 24)      # depthwise units (+ the 16-bit pointwise ones)
    elif dtype == torch.bfloat16:
        # the apply pass of the 16-bit pointwise units; + the depthwise units whose backward is a row-walking kernel (prologue: fd_bstat_table_block)
        assert info["units_finalising_their_own_backward"] >= (20 if info["dw_units_backward_on_row_kernels"] else 10), info
    else:
        assert info["units_finalising_their_own_backward"] == 0
    if dtype == torch.bfloat16:
        assert "dz" in rep
    if name.endswith("sat6"):
        assert harness.LAST_SAT6_FRAC > 0.005, harness.LAST_SAT6_FRAC
    if flags & TOOK_EFFECT_BITS:
        check_train_form_took_effect(kind, name, plan, dtype, flags)


# ---- a passing parity check proves nothing if the bit silently had no effect ------------------------------------------------------------

GEOMETRY_FIELDS = ("th", "tw", "bth", "btw", "d_th", "d_tw", "cb", "pstr", "bpstr", "lds")
TOOK_EFFECT_BITS = (F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16 | F.FD_TUNE_DW_SMALL_TILES | F.FD_TUNE_DW_PITCH4 | F.FD_TUNE_DW_PITCH8 | F.FD_TUNE_DW_WGRAD_TH4 |
                    F.FD_TUNE_NO_PW_PAIRING | F.FD_TUNE_PW_PAIR_TN2)

# (case name, storage type, flags) -> {unit: {field: (value under the flags, value in the default plan)}}, every value derived from fd_train_plan_create /
# dw_bwd_plan / dw_dgrad_rows (csrc/fd_train_impl.h), not from a run.  Maps of TINY at 64 x 64: conv1 32 x 32, conv2 / 3 16 x 16, conv4 / 5 8 x 8, conv6 ... 11
# 4 x 4, conv12 / 13 / decode_conv1 2 x 2, decode_conv2 4 x 4 ... decode_conv5 32 x 32; at 224 x 32: 112 x 16, 56 x 8, 28 x 4, 14 x 2, 7 x 1, decode_conv2 14 x 2,
# decode_conv3 28 x 4.  Depthwise channels of TINY: conv1.0 8, conv5.0 / conv6.0 32, conv7.0 40, decode_conv1.0 48, decode_conv2.0 40, decode_conv3.0 32 (blocks: the
# largest power of two <= the count, at most 32, FD_TUNE_DW_CB16: 16); of RAGGED: decode_conv1.0 112, decode_conv2.0 200.  Pitch: block + 4 dwords (+ 12 with both
# pitch bits).  In a bf16 plan only the LDS-tiled units read these fields: decode_conv1.0 / decode_conv2.0 (the others run on row-walking kernels).
EXPECTED_GEOMETRY = {
    # 8 rows where the balanced count is the map's own height (backward-data tiles taller than a 4 x 4 / 2 x 2 map: one ragged tile); the 16 x 16 output of
    # conv2.0 splits 8 + 8 either way.  NB this case alone does NOT exercise a ragged 8-row tile: at 64 x 64 every map height is a power of two, the bit only makes
    # the backward-data tile exceed the small maps and the arithmetic equals the default plan's.  The ragged LAST tile is the business of the 224 x 32 cases below.
    ("tiny", torch.float32, F.FD_TUNE_DW_TH8): {"conv7.0": {"d_th": (8, 4)}, "conv12.0": {"d_th": (8, 4)}, "decode_conv2.0": {"d_th": (8, 4)}},
    ("ragged", torch.bfloat16, F.FD_TUNE_DW_CB16): {"decode_conv1.0": {"cb": (16, 32), "pstr": (20, 36), "bpstr": (20, 36)}, "decode_conv2.0": {"cb": (16, 32), "pstr": (20, 36)}},
    # the 3x3 stride-1 forward tiles stay at the backward kernels' 8 x 16 instead of 14 x 28 (32 x 32 map) / 14 x 16 (16 x 16 map)
    ("tiny", torch.float32, F.FD_TUNE_DW_SMALL_TILES): {"conv1.0": {"th": (8, 14), "tw": (16, 28)}, "conv3.0": {"th": (8, 14), "tw": (16, 16)}},
    # + 12 dwords of pitch forward and backward; 5x5 weight-gradient tiles of 4 rows instead of 8.  conv1.0's forward patch: (14 + 2) x (28 + 2) = 480 pixels
    ("tiny", torch.float32, F.FD_TUNE_DW_PITCH4 | F.FD_TUNE_DW_PITCH8 | F.FD_TUNE_DW_WGRAD_TH4): {
        "conv1.0": {"pstr": (24, 12), "bpstr": (24, 12), "lds_delta": 480 * 12 * 4}, "decode_conv5.0": {"pstr": (32, 20), "bth": (4, 8)}, "decode_conv3.0": {"pstr": (48, 36), "bth": (4, 8)}},
    ("tiny_tall", torch.float32, F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16): {
        "conv5.0": {"bth": (8, 7), "d_th": (8, 14), "cb": (16, 32), "pstr": (20, 36), "th": (14, 14)},          # 28 rows: 8 + 8 + 8 + 4
        "conv6.0": {"th": (8, 7), "cb": (16, 32)},                                                                # 14 output rows: 8 + 6
        "conv7.0": {"bth": (8, 7), "d_th": (8, 14), "cb": (16, 32)},
        "decode_conv3.0": {"th": (8, 7), "tw": (4, 4), "cb": (16, 32)}},
    ("tiny_tall", torch.bfloat16, F.FD_TUNE_DW_TH8 | F.FD_TUNE_DW_CB16): {"decode_conv2.0": {"th": (8, 7), "cb": (16, 32), "pstr": (20, 36)}, "decode_conv1.0": {"th": (7, 7), "cb": (16, 32)}},
}


def dw_geometry(kind, model, x, dtype, flags):
    """{unit name: {field: value}} of a train plan's depthwise units (private host-only hook fd_train_plan_dw_geometry, csrc/fd_tuning.h)."""
    tp = harness.CTrainPlan(kind, model, x, dtype=dtype, flags=flags)
    try:
        fn = tp.lib.fd_train_plan_dw_geometry
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
        out = {}
        buf = (ctypes.c_int32 * len(GEOMETRY_FIELDS))()
        for i, l in enumerate(tp.layers):
            if l.desc.op == capi.FD_OP_DW:
                assert fn(tp.h, i, buf, len(GEOMETRY_FIELDS)) == len(GEOMETRY_FIELDS), l.name
                out[l.name] = dict(zip(GEOMETRY_FIELDS, list(buf)))
            else:
                assert fn(tp.h, i, buf, len(GEOMETRY_FIELDS)) == -1, l.name
        assert fn(tp.h, len(tp.layers), buf, len(GEOMETRY_FIELDS)) == -1 and fn(tp.h, 1, buf, len(GEOMETRY_FIELDS) - 1) == -1
        return out
    finally:
        tp.close()


def launch_census(model, x, target, dtype, flags):
    """-> (kernel names -- the launch macro's source text, template arguments included -- of one forward + backward of a product train plan on the device, the
    (M, K) of every pointwise unit but the head as the plan holds them).  fd_trace_begin / fd_trace_end: offered by the HIP build only."""
    tp = harness.CTrainPlan("hip", model, x.cuda(), keep=False, dtype=dtype, flags=flags)
    try:
        mk = []
        for i, l in enumerate(tp.layers):
            if l.desc.op == capi.FD_OP_PW and l.desc.cout != 1:
                d = [ctypes.c_int32() for _ in range(4)]
                capi.check(tp.lib, tp.lib.fd_train_layer_tensor(tp.h, i, 0, None, *[ctypes.byref(v) for v in d]), "fd_train_layer_tensor")
                mk.append((d[0].value * d[1].value * d[2].value, l.desc.cin))
        capi.check(tp.lib, tp.lib.fd_trace_begin(), "fd_trace_begin")
        y = tp.forward(x.cuda()).cpu()
        tp.backward(torch.sign(y - target) / y.numel())
        n = ctypes.c_int32(); recs = (capi.TraceRecord * 4096)()
        capi.check(tp.lib, tp.lib.fd_trace_end(torch.cuda.current_stream().cuda_stream, recs, 4096, ctypes.byref(n)), "fd_trace_end")
        return [r.kernel.decode() for r in recs[:n.value]], mk
    finally:
        tp.close()


def pw_units_on_wide_dgrad_tiles(mk):
    """fd_train_bwd_impl.h (launch_pw_bwd_h16): a 16-bit pointwise unit's backward-data GEMM takes 64 x 128 tiles when it has >= 128 input channels and that
    still leaves >= 200 workgroups; in the paired launch only under FD_TUNE_PW_PAIR_TN2.  mk: the units' (M, K) from the plan (launch_census)."""
    return sum(1 for M, K in mk if K >= 128 and -(-M // 64) * -(-K // 128) >= 200)


def check_train_form_took_effect(kind, name, plan, dtype, flags):
    """The plan of a tile-geometry case differs from the default plan in the way its bits promise (fd_train_plan_dw_geometry on both plans against the values
    derived from the plan code); the plan of a pairing case launches what its bit promises (device only: the launch census of fd_trace)."""
    m, x, target = train_local_inputs(name, plan)
    xd = x.to(device_of(kind))
    if (name, dtype, flags) in EXPECTED_GEOMETRY:
        got, default = dw_geometry(kind, m, xd, dtype, flags), dw_geometry(kind, m, xd, dtype, 0)
        for unit, fields in EXPECTED_GEOMETRY[(name, dtype, flags)].items():
            assert any(k == "lds_delta" or v[0] != v[1] for k, v in fields.items()), "%s: no expected field differs from the default plan" % unit
            for field, want in fields.items():
                if field == "lds_delta":
                    assert got[unit]["lds"] - default[unit]["lds"] == want, (unit, got[unit], default[unit])
                    continue
                assert (got[unit][field], default[unit][field]) == want, (unit, field, got[unit], default[unit])
    else:
        assert not flags & (TOOK_EFFECT_BITS & ~(F.FD_TUNE_NO_PW_PAIRING | F.FD_TUNE_PW_PAIR_TN2)), "a tile-geometry case without expected values"
    if flags & (F.FD_TUNE_NO_PW_PAIRING | F.FD_TUNE_PW_PAIR_TN2) and kind == "hip":
        count = lambda names, key: sum(1 for k in names if key in k)
        (names, mk), (base, _) = launch_census(m, x, target, dtype, flags), launch_census(m, x, target, dtype, 0)
        assert dtype == torch.bfloat16 and len(mk) == 18
        tn2 = lambda ns: sum(1 for k in ns if "fd_pw_bwd_h16<" in k and k.rstrip(")").rstrip().endswith(", 2>"))       # the 64 x 128 instance: last template argument 2
        # default: the two GEMMs of each of the 18 pointwise units (all but the head) share one launch, all on 64 x 64 backward-data tiles
        assert (count(base, "fd_pw_bwd_h16<"), count(base, "fd_pw_wgrad_h16<"), count(base, "fd_pw_dgrad_h16<"), tn2(base)) == (18, 0, 0, 0), base
        if flags & F.FD_TUNE_NO_PW_PAIRING:
            # ... each on its own, while the depthwise units keep their forms (paired / single-staging / row-walking launches as in the default plan)
            assert (count(names, "fd_pw_bwd_h16<"), count(names, "fd_pw_wgrad_h16<"), count(names, "fd_pw_dgrad_h16<")) == (0, 18, 18), names
            assert [k for k in names if "fd_dw" in k] == [k for k in base if "fd_dw" in k] and len(names) == len(base) + 18
        if flags & F.FD_TUNE_PW_PAIR_TN2:
            # the paired launch's 64 x 128 instance on exactly the units the rule selects, the 64 x 64 one on the others.  The case on TN2 at 2 x 160 x 224 is the one
            # where the bit changes a launch (conv3.3: M = 4480, K = 264); RAGGED at 64 x 64 (the issue's case) selects none: conv5.3, K = 144, has 4 of the 200 workgroups
            wide = pw_units_on_wide_dgrad_tiles(mk)
            assert wide == (1 if plan is TN2 else 0), mk
            assert count(names, "fd_pw_bwd_h16<") == 18 and tn2(names) == wide, names


STAT_ROWS_DTYPES = [torch.float32, torch.bfloat16]


def check_statistics_rows_cover_large_and_small_magnitudes(kind, dtype):
    """The BatchNorm statistics rows place every fp32 partial sum exactly into one of three integer accumulators chosen by its binary exponent
    (csrc/fd_device.h: fd_stat_add; forward bins below 2^-8 / below 2^16 / above, backward below 2^-32 / below 2^-8 / above).  Conv weights scaled by
    1e3 resp. 1e-3 (train-mode BatchNorm removes the scale from everything downstream, and divides that unit's weight gradient by it) push the sums of
    z, z^2 of alternating units into the highest and the lowest forward bin, and their gradients' sums across the backward bins; the layer-local fp64
    check must hold exactly as for the unscaled model."""
    t0 = time.time()
    m = small_model(TINY[0], TINY[1], seed=3)
    # (only units whose maps hold >= 128 values per channel at this test size: with the 8 values per channel of the 2 x 2 maps and no eps to hide
    # behind -- var >> eps once z is scaled by 1e3 -- the single-pass variance E[z^2] - mean^2 of ANY fp32 implementation loses digits in channels whose
    # |mean| >> std; that is a property of the small test geometry, not of the accumulation under test)
    scaled = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.Conv2d) and n.split(".")[0] in ("conv0", "conv1", "conv2", "conv3", "decode_conv4", "decode_conv5")]
    assert len(scaled) == 11
    for k, n in enumerate(scaled):
        dict(m.named_modules())[n].weight.data.mul_(1e3 if k % 2 == 0 else 1e-3)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 64, 64, generator=g)
    target = 2.0 + torch.rand(2, 1, 64, 64, generator=g)
    rep = harness.local_train_parity(kind, m, x, target, device_of(kind), dtype=dtype)
    _note_local(kind, "statistics_rows_cover_large_and_small_magnitudes", str(dtype).split(".")[-1], t0, rep, dtype)
    assert_local_parity(rep, dtype)


SKIP_CONCAT_TRAIN_CASES = [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, F.FD_TUNE_DW_BWD1)]


def check_skip_concat_train_step_layer_local(kind, dtype, flags):
    """Row f-3: train step of the concatenating sibling (depthwise MODE 3 in the train forward, backward-data and backward-weights
    kernels: two channel ranges read from / differentiated into two tensors), small widths, layer-local fp64 check."""
    t0 = time.time()
    models = inputs.product_models()
    torch.manual_seed(41)
    enc = (8, 32, 24, 32, 32, 32, 40, 40, 40, 40, 40, 40, 48, 48)          # skips: enc[1] = enc[3] = enc[5] = 32; producers dec[1..3] = 32 (multiples of 32)
    m = harness.randomize_bn(models.MobileNetSkipConcat((64, 64), pretrained=False, channels=(enc, (40, 32, 32, 32, 8, 1))), 42)
    g = torch.Generator().manual_seed(43)
    x = torch.rand(2, 3, 64, 64, generator=g)
    target = 2.0 + torch.rand(2, 1, 64, 64, generator=g)
    rep = harness.local_train_parity(kind, m, x, target, device_of(kind), dtype=dtype, flags=flags)     # (DW_BWD1: MODE 3 through the single-staging backward kernel)
    _note_local(kind, "skip_concat_train_step_layer_local", "%s-%s" % (str(dtype).split(".")[-1], flag_names(flags)), t0, rep, dtype)
    assert_local_parity(rep, dtype)
