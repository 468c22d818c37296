"""fd_pw_gemm16_f32 with its weight fragments loaded straight into registers (template parameter BREG, csrc/fd_kernels_gemm16_f32.h) against the
form that stages the weight rows through the LDS ring (FD_TUNE_G16_B_LDS): the two read the same bytes and issue the same MFMAs in the same
order, so every stored tensor must be BITWISE equal.  TEST INFRASTRUCTURE ONLY, shared by tests/test_emu_gemm16_breg.py (kind = "emu") and
tests/test_gpu_gemm16_breg.py (kind = "hip") as tests/forms.py is by the form matrix: same models, seeds, shapes and assertions in both tiers."""
import ctypes
import time

import numpy as np
import torch

import forms
import harness
from forms import F, G16, device_of, note, small_model

BREG_TMS = {"7", "4"}            # row-tile counts the plan runs in the register form (g16_breg_pick, csrc/fd_plan_select.h); TM = 13 keeps the LDS form
REG_NOTE = "weight fragments in registers"


def _tm(line):
    return line.split("TM=")[1].split(":")[0]


def _pair(kind, m, x, flags=0, **kw):
    """(plan in the product's form, plan with every gemm16 launch in the LDS form), both with FD_TUNE_FORCE_GEMM16 and one buffer per layer"""
    dev = device_of(kind)
    return (harness.CPlan(kind, m, x.to(dev), flags=F.FD_TUNE_FORCE_GEMM16 | flags, **kw),
            harness.CPlan(kind, m, x.to(dev), flags=F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_G16_B_LDS | flags, **kw))


def _assert_forms_differ(info_reg, info_lds):
    """the LDS-form plan has no register-form launch; the product's plan has one on every gemm16 layer with TM in BREG_TMS and only there; nothing
    else differs (same tiles, same fusions).  Returns the gemm16 lines of the product's plan."""
    assert len(info_reg) == len(info_lds)
    used = [(a, b) for a, b in zip(info_reg, info_lds) if a.startswith("pw_gemm16")]
    assert used and all(b.startswith("pw_gemm16") for _, b in used)
    assert not any(REG_NOTE in b for b in info_lds), info_lds
    for a, b in used:
        assert (REG_NOTE in a) == (_tm(a) in BREG_TMS), a
        assert a.split(" lds=")[0] == b.split(" lds=")[0] and ("fused dw" in a) == ("fused dw" in b), (a, b)      # same tile, same fusion
    assert any(REG_NOTE in a for a, _ in used), info_reg
    assert [a for a, b in zip(info_reg, info_lds) if not a.startswith("pw_gemm16")] == [b for b in info_lds if not b.startswith("pw_gemm16")]
    return [a for a, _ in used]


def _assert_bitwise(p_reg, p_lds, x):
    dev = p_reg.dev
    y_reg, y_lds = p_reg.forward(x.to(dev)), p_lds.forward(x.to(dev))
    assert torch.isfinite(y_reg).all()
    assert np.array_equal(harness.bits_of(y_reg), harness.bits_of(y_lds))
    stored = 0
    for i in range(len(p_reg.layers)):
        a, b = p_reg.raw(i), p_lds.raw(i)
        assert (a is None) == (b is None), i
        if a is not None:
            assert a[2] == b[2] and np.array_equal(a[0], b[0]), "layer %d differs between the register form and the LDS form" % i
            stored += 1
    return stored


def check_bitwise_ab(kind, name, plan, b, hw):
    """forms.GEMM16_CASES under FD_TUNE_FORCE_GEMM16: TM = 13 / 7 / 4, strides below the tile, ragged M, N (not a multiple of 64) and K (not a multiple of
    32, i.e. the zero padding of the weight rows is what the register loads read beyond K); every stored layer tensor and the output."""
    t0 = time.time()
    h, w = (hw, hw) if isinstance(hw, int) else hw
    m = small_model(plan[0], plan[1], seed=21).eval()
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(8))
    p_reg, p_lds = _pair(kind, m, x)
    used = _assert_forms_differ(p_reg.info(), p_lds.info())
    assert len(used) == 18, used
    if name == "ragged":
        assert {_tm(s) for s in used} == {"13", "7", "4"}, used
    stored = _assert_bitwise(p_reg, p_lds, x)
    note(kind, "gemm16_breg_bitwise", name, t0, register_form=sum(REG_NOTE in s for s in used), lds_form=sum(REG_NOTE not in s for s in used), stored_tensors=stored)
    p_reg.close(); p_lds.close()


# the product's conv13.3 form: 7x7 maps, two frames per workgroup (112 x 64 tile, stride 98) with the fused 5x5 consumer, whose zero-bordered
# image (243 rows x 272 B = 66 096 B) is larger than the A-only ring (4 x 112 x 128 B = 57 344 B); and decode_conv1.1's: one 7x7 frame per
# workgroup (64 x 64 tile, stride 49) with the fused 5x5 on the nearest-x2 upsampling.  7x7 is the 1/32 map of a 224 x 224 input; the forcing
# bit takes TM = 7 for 64 < M <= 112 and TM = 4 below, so batch 2 / batch 1 of the thin model are the smallest cases.
THIN = ((8, 8, 8, 8, 8, 8, 16, 16, 16, 16, 16, 24, 40, 48), (40, 8, 8, 8, 8, 1))      # 8 channels on the large maps (the emulator walks every pixel); conv13.3: K = 40 (ragged), N = 48
FUSED_CASES = [("conv13_form", 2, "TM=7: 112x64 tile, stride 98", "fused dw k5", "k5 s1"), ("decode_conv1_form", 1, "TM=4: 64x64 tile, stride 49", "fused dw k5", "k5 s1 on up2")]


def check_fused_consumer_image(kind, name, b, tile, fused, dw):
    t0 = time.time()
    m = small_model(THIN[0], THIN[1], seed=23).eval()
    x = torch.rand(b, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    p_reg, p_lds = _pair(kind, m, x, fill=0xFF, guard=4096)        # 0xFF bytes: every float of the workspace (and of the guards around it) starts as a NaN
    info = p_reg.info()
    _assert_forms_differ(info, p_lds.info())
    line = [s for s in info if tile in s and fused in s]
    assert line and all(REG_NOTE in s for s in line), info
    assert any("(dw %s evaluated in the epilogue" % dw in s for s in info), info
    lds = int(line[0].split(" lds=")[1].split(",")[0].split(" ")[0])
    if name == "conv13_form":
        assert lds == 243 * 68 * 4 > 4 * 112 * 128, line                # the launch asks for the image, not for the ring
    stored = _assert_bitwise(p_reg, p_lds, x)
    assert p_reg.bad_guards() == 0 and p_lds.bad_guards() == 0
    note(kind, "gemm16_breg_fused_image", name, t0, lds=lds, stored_tensors=stored)
    p_reg.close(); p_lds.close()


def check_short_k(kind):
    """K = 32 and K = 64: one and two K tiles, fewer than the ring's stages and than the depth of the weight-fragment prefetch.  G16 at 1 x 3 x 32 x 32:
    conv2.3 (32 -> 64) and conv3.3 (64 -> 64) run on 8 x 8 maps, M = 64, TM = 4."""
    t0 = time.time()
    m = small_model(G16[0], G16[1], seed=25).eval()
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(12))
    p_reg, p_lds = _pair(kind, m, x)
    used = _assert_forms_differ(p_reg.info(), p_lds.info())
    for k in (32, 64):
        assert any(REG_NOTE in s and " K=%d " % k in s for s in used), used
    stored = _assert_bitwise(p_reg, p_lds, x)
    note(kind, "gemm16_breg_short_k", "g16", t0, stored_tensors=stored)
    p_reg.close(); p_lds.close()


# Reductions of 8 or more K tiles: the branch-free path of the register form (its own prologue, the four-step steady loop with the leaders' counted
# waits, and behind it either the last four tiles -- K a multiple of four tiles -- or the run-time steps), which the product's launches take (K = 256 /
# 512 / 1024) and which none of the models above reaches (their K stay below 256).  LONGK at 20 x 3 x 32 x 32: the 1/16 maps are 2 x 2, M = 80 -> TM = 7;
# the 1/32 maps 1 x 1, M = 20 -> TM = 4; the wide layers sit only there, so the emulator's case stays at seconds.
#   conv7.3   K = 256 (T = 8:  steady loop once, last four)         N = 288   TM = 7
#   conv8.3   K = 288 (T = 9:  steady loop once, 5 run-time steps)  N = 16    TM = 7
#   conv12.3  K = 512 (T = 16: steady loop three times, last four)  N = 408   TM = 4
#   conv13.3  K = 408 (T = 13, ragged: two loops, 5 run-time steps) N = 16    TM = 4
LONGK = ((8, 8, 8, 8, 8, 8, 256, 288, 16, 16, 16, 512, 408, 16), (16, 8, 8, 8, 8, 1))
LONGK_LAYERS = [("TM=7", 288, 256), ("TM=7", 16, 288), ("TM=4", 408, 512), ("TM=4", 16, 408)]


def check_long_k(kind):
    t0 = time.time()
    m = small_model(LONGK[0], LONGK[1], seed=29).eval()
    x = torch.rand(20, 3, 32, 32, generator=torch.Generator().manual_seed(14))
    p_reg, p_lds = _pair(kind, m, x, fill=0xFF, guard=4096)
    used = _assert_forms_differ(p_reg.info(), p_lds.info())
    for tm, n, k in LONGK_LAYERS:
        assert any(REG_NOTE in s and ("<%s:" % tm) in s and (" N=%d K=%d " % (n, k)) in s for s in used), (tm, n, k, used)
    stored = _assert_bitwise(p_reg, p_lds, x)
    assert p_reg.bad_guards() == 0 and p_lds.bad_guards() == 0
    note(kind, "gemm16_breg_long_k", "longk", t0, stored_tensors=stored)
    p_reg.close(); p_lds.close()


def check_train_forward(kind):
    """Two SGD steps of the G16 model (every pointwise reduction a multiple of 32: the train mode of the kernel, on live weights) in fp32, with and
    without the bit.  Train plans keep the weight rows in the LDS ring (the register form lost there and is not built: csrc/fd_train_impl.h), so the
    bit must be accepted and change nothing: the same unit kernels, equal losses, and the raw output and BatchNorm table (the statistics rows,
    finalised) of every unit whose forward runs on the kernel bit for bit."""
    import copy
    from fastdepth_hip.train import TrainEngine, _TrainPlan
    t0 = time.time()
    L = harness.get_lib(kind)
    dev = device_of(kind)
    base = small_model(G16[0], G16[1], seed=27).train()
    g = torch.Generator().manual_seed(13)
    x, tgt = torch.rand(2, 3, 32, 32, generator=g).to(dev), (2.0 + torch.rand(2, 1, 32, 32, generator=g)).to(dev)      # maps of 16 x 16 ... 1 x 1: M = 512 ... 2, TM = 13 and 4

    def run(flags):
        saved = _TrainPlan.default_flags
        _TrainPlan.default_flags = flags
        try:
            eng = TrainEngine(copy.deepcopy(base).to(dev), lr=0.01, momentum=0.9, weight_decay=1e-4, **({"_library": L} if kind == "emu" else {}))
            losses = [float(eng.step(x, tgt)) for _ in range(2)]
        finally:
            _TrainPlan.default_flags = saved
        plan = eng._plan
        units = [L.fd_train_plan_unit_kernels(plan.handle, i) for i in range(eng.n)]
        got = []
        for i in [i for i, u in enumerate(units) if u > 0 and u & 1]:
            for which in (0, 2):
                ptr = ctypes.c_void_p()
                d = [ctypes.c_int32() for _ in range(4)]
                harness.capi.check(L, L.fd_train_layer_tensor(plan.handle, i, which, ctypes.byref(ptr), *[ctypes.byref(v) for v in d]), "fd_train_layer_tensor")
                n, h, w, c = [v.value for v in d]
                off = ptr.value - plan.workspace.data_ptr()
                got.append(plan.workspace[off:off + n * h * w * c * 4].clone().cpu())
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return losses, units, got

    l_reg, u_reg, t_reg = run(F.FD_TUNE_FORCE_GEMM16)
    l_lds, u_lds, t_lds = run(F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_G16_B_LDS)
    assert u_reg == u_lds and sum(1 for u in u_reg if u > 0 and u & 1) >= 9, (u_reg, u_lds)
    assert l_reg == l_lds and all(v == v for v in l_reg), (l_reg, l_lds)
    assert len(t_reg) == len(t_lds) and all(torch.equal(a, b) for a, b in zip(t_reg, t_lds))
    note(kind, "gemm16_breg_train_forward", "g16", t0, losses=l_reg, gemm16_units=sum(1 for u in u_reg if u > 0 and u & 1))
