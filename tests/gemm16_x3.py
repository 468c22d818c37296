"""The split-bf16 form of fd_pw_gemm16_f32 (template parameter X3, csrc/fd_kernels_gemm16_x3.h): the fp32 product as six bf16 MFMAs on three bf16
planes of each operand.  The producer of the A operand -- the depthwise stage in a gemm16 epilogue -- writes the planes, the weights' are packed once.
TEST INFRASTRUCTURE ONLY, shared by tests/test_emu_gemm16_x3.py (kind = "emu") and tests/test_gpu_gemm16_x3.py (kind = "hip"): same models, seeds,
shapes and assertions in both tiers.  FD_TUNE_FORCE_G16_X3 puts every eligible layer on the form, FD_TUNE_NO_G16_X3 none (the fp32 forms)."""
import ctypes
import time

import numpy as np
import torch

import forms
import harness
from forms import F, G16, device_of, note, small_model
from gemm16_breg import LONGK, THIN

X3_NOTE = " [split-bf16 form]"       # _info() appends it where the kernel symbol is the X3 form (the info lines themselves do not change with the form)
FORCE = F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_FORCE_G16_X3
FP32_LDS = F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_NO_G16_X3 | F.FD_TUNE_G16_B_LDS        # the fp32 LDS form: the reference of the error bound

# K = 1024 at M = one tile (steady state of the ring plus its drain): conv12.3 reduces 1024 channels on the 1 x 1 maps of 20 frames (TM = 4), conv11.3 produces them
DEEPK = ((8, 8, 8, 8, 8, 8, 16, 16, 16, 16, 16, 1024, 16, 16), (16, 8, 8, 8, 8, 1))
# name, widths, batch, (h, w): every TM (13 / 7 / 4); consumers none, dw3 s1, dw3 s2, dw5, dw5 on up2; one and two frames per workgroup; a short last M
# tile; N % 64 != 0; K = 32 / 64 (shorter than the ring), K = 40 (ragged, padded to 64), K up to 1024
# short_m: five frames of 160 x 288.  conv11.3 works on 10 x 18 maps (M = 900: five workgroups of one whole frame each, so its epilogue evaluates conv12.0,
# 3x3 stride 2, and stores conv12.3's A planes); conv12.3 has M = 5 x 45 = 225 rows: two M tiles of the balanced stride 113, the last one 112 rows -- there
# its LDS-DMA source rows clamp at M - 1 and its epilogue stores rows = M - m0
CASES = [("ragged", forms.RAGGED, 2, (32, 96)), ("tiny", forms.TINY, 2, (64, 64)), ("thin_two_frames", THIN, 2, (224, 224)), ("thin_one_frame", THIN, 1, (224, 224)),
         ("g16_short_k", G16, 1, (32, 32)), ("longk", LONGK, 20, (32, 32)), ("deepk", DEEPK, 20, (32, 32)),
         ("short_m", THIN, 5, (160, 288))]
PLANE_CASES = [("tiny", forms.TINY, 2, (64, 64)), ("ragged", forms.RAGGED, 2, (32, 96))]


def _model_x(plan, b, hw, seed=31):
    m = small_model(plan[0], plan[1], seed=seed).eval()
    x = torch.rand(b, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(seed + 1))
    return m, x


def _info(p):
    """fd_plan_kernel_info per layer, tagged with X3_NOTE where fd_plan_kernel_symbol names the split-bf16 form (last template argument of fd_pw_gemm16_f32 != 0)"""
    syms = [p.lib.fd_plan_kernel_symbol(p.h, i).decode() for i in range(p.lib.fd_plan_num_kernels(p.h))]
    return [s + (X3_NOTE if y.startswith("fd_pw_gemm16_f32<") and not y.endswith(", 0>") else "") for s, y in zip(p.info(), syms)]


def _x3(p, i):
    """the hook of csrc/fd_tuning.h: ([pointers], [dims]) of layer i"""
    out, dims = (ctypes.c_void_p * 5)(), (ctypes.c_int64 * 5)()
    assert p.lib.fd_plan_x3_tensors(p.h, i, out, dims) == 0
    return list(out), list(dims)


def _bytes(p, ptr, n):
    off = ptr - p.ws.data_ptr()
    assert 0 <= off and off + n <= p.ws.numel()
    return p.ws[off:off + n].cpu().numpy().copy()


def _bf16_as_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def _a_planes(p, i):
    """(hi, mid, lo) as fp32 arrays [m][k32] from the K-tile-major planes of depthwise layer i, its fp32 tensor [m][c] or None; None if it stores no planes"""
    ptr, dims = _x3(p, i)
    if not ptr[0]:
        return None
    m, k32 = dims[0], dims[1]
    raw = _bytes(p, ptr[0], m * k32 * 6).view(np.uint16).reshape(k32 // 32, 3, m, 32)
    parts = [_bf16_as_f32(np.ascontiguousarray(raw[:, j].transpose(1, 0, 2)).reshape(m, k32)) for j in range(3)]
    f32 = None
    if ptr[1]:
        c = p.layers[i].desc.cout
        f32 = _bytes(p, ptr[1], m * c * 4).view(np.float32).reshape(m, c)
    return parts, f32


def _w_planes(p, i):
    ptr, dims = _x3(p, i)
    if not ptr[2]:
        return None
    n, k32 = dims[2], dims[3]
    planes = _bf16_as_f32(_bytes(p, ptr[2], n * k32 * 6).view(np.uint16).reshape(3, n, k32))
    w = _bytes(p, ptr[3], n * k32 * 4).view(np.float32).reshape(n, k32)
    b = _bytes(p, ptr[4], n * 4).view(np.float32)
    return planes, w, b, dims[4]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_planes(kind, name, plan, b, hw):
    """Every producer store mode on a poisoned workspace (every byte 0xFF: NaNs).  KEEP_ACTIVATIONS plan: the producer stores the fp32 tensor AND the
    planes; (hi + mid) + lo evaluated in fp32 is the fp32 tensor bit for bit, the pad columns up to K32 are zero in all three planes.  The plan that
    stores the planes only computes the same network output bit for bit.  Weight planes: they sum to the folded fp32 weight bit for bit, all three parts
    carry the sign of w, no part is zero unless w is."""
    t0 = time.time()
    dev = device_of(kind)
    m, x = _model_x(plan, b, hw)
    pk = harness.CPlan(kind, m, x.to(dev), flags=FORCE, fill=0xFF, guard=4096)
    po = harness.CPlan(kind, m, x.to(dev), keep=False, flags=FORCE, fill=0xFF, guard=4096)
    yk, yo = pk.forward(x.to(dev)), po.forward(x.to(dev))
    assert torch.isfinite(yk).all()
    assert np.array_equal(harness.bits_of(yk), harness.bits_of(yo)), "planes-only plan differs from the plan that stores both"
    for p in (pk, po):            # both store modes have producers of planes; only the KEEP_ACTIVATIONS plan stores the fp32 tensor next to them
        got = [_x3(p, i)[0] for i in range(len(p.layers))]
        assert sum(1 for q in got if q[0]) >= 8 and all(bool(q[1]) == (p is pk) for q in got if q[0])
    producers = weights = 0
    for i in range(len(pk.layers)):
        got = _a_planes(pk, i)
        if got is not None:
            (hi, mid, lo), f32 = got
            c = f32.shape[1]
            s = (hi + mid).astype(np.float32) + lo
            assert np.array_equal(_bits(s[:, :c]), _bits(f32)), "layer %d: (hi + mid) + lo is not the fp32 output" % i
            for part in (hi, mid, lo):
                assert not _bits(part[:, c:]).any(), "layer %d: pad columns are not zero" % i
            producers += 1
        gw = _w_planes(pk, i)
        if gw is not None:
            planes, w, _, _ = gw
            s = (planes[0] + planes[1]).astype(np.float32) + planes[2]
            assert np.array_equal(_bits(s), _bits(w)), "layer %d: weight planes do not sum to the folded weight" % i
            nz = w != 0
            for part in planes:
                assert np.array_equal(np.signbit(part[nz]), np.signbit(w[nz])), i
                assert (part[nz] != 0).all() and not _bits(part[~nz]).any(), i
            weights += 1
    assert producers >= 8 and weights >= 10, (producers, weights)
    assert pk.bad_guards() == 0 and po.bad_guards() == 0
    note(kind, "gemm16_x3_planes", name, t0, producers=producers, weight_layers=weights)
    pk.close(); po.close()


def _layer_errors(p):
    """[(layer, info, rel_err of its stored output against the fp64 product of its own stored fp32 operands)] for the gemm16 layers whose A is also stored as fp32"""
    res, info = [], _info(p)
    for i, l in enumerate(p.layers):
        gw = _w_planes(p, i)
        if gw is None or not info[i].startswith("pw_gemm16"):
            continue
        _, w, bias, _ = gw
        a = p.tap(l.desc.src).permute(0, 2, 3, 1).reshape(-1, l.desc.cin).double().numpy()
        ref = a @ w[:, :l.desc.cin].astype(np.float64).T + bias.astype(np.float64)
        ref = np.maximum(ref, 0.0) if l.desc.act != F.FD_ACT_NONE else ref
        ref = np.minimum(ref, 6.0) if l.desc.act == F.FD_ACT_RELU6 else ref
        out = p.tap(i).permute(0, 2, 3, 1).reshape(-1, l.desc.cout).double().numpy()
        res.append((i, info[i], harness.rel_err(out, ref)))
    return res


def check_gemm_against_fp64(kind, name, plan, b, hw):
    """rel_err of the split-bf16 form against the fp64 product of the same fp32 operands <= 2 x the rel_err of the fp32 LDS form on that layer.  The CPU model
    (tools/x3_numerics.py) gives ratios of 0.8 - 1.2; the factor 2 covers the hardware MFMA's own accumulation order.  Determinism: a second run and a
    permutation of the frames give the same bits."""
    t0 = time.time()
    dev = device_of(kind)
    m, x = _model_x(plan, b, hw)
    px = harness.CPlan(kind, m, x.to(dev), flags=FORCE, fill=0xFF, guard=4096)
    pl = harness.CPlan(kind, m, x.to(dev), flags=FP32_LDS)
    y1 = px.forward(x.to(dev))
    ex = {i: (s, e) for i, s, e in _layer_errors(px) if X3_NOTE in s}
    assert ex, _info(px)
    pl.forward(x.to(dev))
    el = {i: e for i, _, e in _layer_errors(pl)}
    assert not any(X3_NOTE in s for s in _info(pl))
    ratios = []
    for i, (s, e) in sorted(ex.items()):
        print("X3RATIO %s %s layer %d %s: x3 %.3g fp32-lds %.3g ratio %.2f" % (kind, name, i, s.split(" tiles=")[0], e, el[i], e / max(el[i], 1e-30)))
        ratios.append(e / max(el[i], 1e-30))
    for i, (s, e) in sorted(ex.items()):
        assert e <= 2.0 * el[i], (i, s, e, el[i])
    y2 = px.forward(x.to(dev))
    assert np.array_equal(harness.bits_of(y1), harness.bits_of(y2)), "two runs differ"
    if b > 1:
        perm = torch.arange(b - 1, -1, -1)
        y3 = px.forward(x[perm].to(dev))
        assert np.array_equal(harness.bits_of(y3), harness.bits_of(y1[perm.to(dev)])), "permuting the frames does not permute the output"
    assert px.bad_guards() == 0
    note(kind, "gemm16_x3_fp64", name, t0, layers=len(ex), worst_ratio=max(ratios), tms=sorted({s.split("TM=")[1].split(":")[0] for s, _ in ex.values()}))
    px.close(); pl.close()
    return ex


def check_case_coverage(kind):
    """the cases above reach every path the issue lists (plan geometry only: no forward)"""
    dev = device_of(kind)
    seen = set()
    for name, plan, b, hw in CASES:
        m, x = _model_x(plan, b, hw)
        p = harness.CPlan(kind, m, x.to(dev), flags=FORCE, pack=False)
        info = _info(p)
        for i, s in enumerate(info):
            if X3_NOTE not in s:
                continue
            tm = s.split("TM=")[1].split(":")[0]
            cons = "none"
            if "fused dw" in s:
                j = int(s.split("of layer ")[1].split()[0])
                cons = info[j].split("(dw ")[1].split(" evaluated")[0]
            seen.add((tm, cons))
            k, n, mm = int(s.split(" K=")[1].split()[0]), int(s.split(" N=")[1].split()[0]), int(s.split(" M=")[1].split()[0])
            stride = int(s.split("stride ")[1].split(">")[0])
            seen.add("k%d" % k if k in (32, 64, 40, 1024) else "k")
            if n % 64:
                seen.add("ragged_n")
            if mm % stride:
                seen.add("short_last_m_tile")
            if "fused dw" in s and stride in (98, 392):
                seen.add("two_frames")
        p.close()
    for tm in ("13", "7", "4"):
        assert any(isinstance(q, tuple) and q[0] == tm for q in seen), (tm, seen)
    for cons in ("none", "k3 s1", "k3 s2", "k5 s1", "k5 s1 on up2"):
        assert any(isinstance(q, tuple) and q[1] == cons for q in seen), (cons, seen)
    for tag in ("k32", "k64", "k40", "k1024", "ragged_n", "two_frames", "short_last_m_tile"):
        assert tag in seen, (tag, seen)


def _cls(t):
    t = torch.as_tensor(t)
    return torch.where(torch.isnan(t), 3, torch.where(torch.isposinf(t), 1, torch.where(torch.isneginf(t), 2, 0)))


def _special_weights(m):
    """every pointwise layer: folded weights of output channel 0 (columns 4, 5, 6) that are exact in bf16 (0.5, -2) and a zero, beside the random ones of mixed sign.  The
    BatchNorm of that channel folds to the scale 1 exactly: gamma / sqrtf(var + eps) = 4096 / sqrtf(2^24), the eps is below half an ulp of 2^24"""
    with torch.no_grad():
        for l in harness.layers_of(m):
            if l.conv.kernel_size == (1, 1) and l.conv.weight.shape[0] > 1:
                w = l.conv.weight.view(-1)
                w[4], w[5], w[6] = 0.5, -2.0, 0.0
                l.bn.weight[0], l.bn.running_var[0] = 4096.0, 2.0 ** 24


def _stored_f32(p, i):
    """layer i's stored fp32 tensor as a writable [m][c] view of the workspace (on the plan's device)"""
    ptr, d = ctypes.c_void_p(), [ctypes.c_int32() for _ in range(4)]
    F.check(p.lib, p.lib.fd_layer_output(p.h, i, ctypes.byref(ptr), *[ctypes.byref(v) for v in d]), "fd_layer_output")
    n, h, w, c = [v.value for v in d]
    off = ptr.value - p.ws.data_ptr()
    return p.ws[off:off + n * h * w * c * 4].view(torch.float32).view(n * h * w, c)


BF16_BITS = {float("inf"): 0x7F80, float("-inf"): 0xFF80 - 0x10000}       # (as int16; NaN below)


def _poke(p, src, row, col, val):
    """element (row, col) of depthwise layer src's stored output becomes the non-finite `val`: in its fp32 tensor and, where it stores planes, as (val, 0, 0) --
    what its store mode writes for a non-finite value"""
    _stored_f32(p, src)[row, col] = val
    ptr, dims = _x3(p, src)
    if ptr[0]:
        mm, k32 = dims[0], dims[1]
        off = ptr[0] - p.ws.data_ptr()
        pv = p.ws[off:off + mm * k32 * 6].view(torch.int16).view(k32 // 32, 3, mm, 32)
        pv[col // 32, 0, row, col % 32] = BF16_BITS.get(val, 0x7FC0)
        pv[col // 32, 1, row, col % 32] = 0
        pv[col // 32, 2, row, col % 32] = 0


def check_nonfinite_a_rows(kind, name, plan, b, hw):
    """The GEMM alone (fd_plan_run_gemm16_layer) on A rows that hold +Inf, -Inf and NaN at the corners and in the middle -- no producer of a plan lets -Inf
    through, its depthwise stage clamps at 0 -- against the fp32 LDS form on the same rows.  Weights: random of mixed sign, and 0.5, -2 (exact in bf16: their
    mid and lo parts are the 2^-120 filler) and a zero in output channel 0, opposite the poisoned columns.  Per output element the class (finite, +Inf, -Inf,
    NaN) is the fp32 form's and the fp64 product's; the finite elements keep the bound of check_gemm_against_fp64: rel_err against the fp64 product <= 2 x the fp32 LDS form's."""
    # (the poisoned columns start at 4 and end at c - 1: where K is no multiple of 32 the fp32 forms read a row's FIRST 16-byte chunk again for the chunks beyond
    # K, against zero weights -- fd_kernels_gemm16_f32.h, `ragged_k` -- so a non-finite value in columns 0 - 3 of such a row makes the whole fp32-form row NaN.
    # The split-bf16 form reads zero planes there and has no such case; the reference of this check is kept clear of it)
    t0 = time.time()
    dev = device_of(kind)
    m, x = _model_x(plan, b, hw, seed=37)
    _special_weights(m)
    px = harness.CPlan(kind, m, x.to(dev), flags=FORCE)
    pl = harness.CPlan(kind, m, x.to(dev), flags=FP32_LDS)
    px.forward(x.to(dev)); pl.forward(x.to(dev))
    forced = [i for i, s in enumerate(_info(px)) if X3_NOTE in s]
    assert forced and not any(X3_NOTE in s for s in _info(pl))
    inf = float("inf")
    worst = 0.0
    for i in reversed(forced):        # (last layer first: a launch with a fused consumer rewrites the A rows of the layer after the next)
        d = px.layers[i].desc
        planes, w, bias, on_form = _w_planes(px, i)
        assert on_form == 1 and tuple(w[0, 4:7]) == (0.5, -2.0, 0.0), (i, w[0, 4:7])
        for part in planes[1:]:       # mid and lo of 0.5 and -2 are the filler, of the zero weight zero
            assert abs(part[0, 4]) == 2.0 ** -120 and abs(part[0, 5]) == 2.0 ** -120 and part[0, 6] == 0, (i, part[0, 4:7])
        mm, c = _stored_f32(px, d.src).shape
        spots = [(0, 4, inf), (1, 5, -inf), (mm // 2, 6, inf), (mm // 2 + 1, c // 2, -inf), (mm - 1, c - 1, float("nan"))]
        assert len({r for r, _, _ in spots}) == 5 and c >= 8, (mm, c)
        for p in (px, pl):
            for r, k, v in spots:
                _poke(p, d.src, r, k, v)
        (hi, mid, lo), a32 = _a_planes(px, d.src)
        assert np.isposinf(hi).any() and np.isneginf(hi).any() and np.isnan(hi).any(), i
        bad = ~np.isfinite(a32)
        assert bad.sum() == 5 and np.array_equal(_cls(hi[:, :c]).numpy(), _cls(a32).numpy()) and not mid[:, :c][bad].any() and not lo[:, :c][bad].any(), i
        outs = []
        for p in (px, pl):
            assert p.lib.fd_plan_run_gemm16_layer(p.h, i, p.stream) == 0
            if dev.type == "cuda":
                torch.cuda.synchronize()
            outs.append(p.tap(i).permute(0, 2, 3, 1).reshape(mm, d.cout).double())
        cx, cl = _cls(outs[0]), _cls(outs[1])
        assert torch.equal(cx, cl), "layer %d: classes differ from the fp32 form's at %s" % (i, torch.nonzero(cx != cl)[:8].tolist())
        # output channel 0: +Inf * 0.5 and -Inf * -2 are +Inf, +Inf * 0 is NaN.  The layer's own activation then clamps: ReLU6 turns +Inf into 6, both turn -Inf
        # into 0 -- such elements count as finite ones, and must equal the reference's
        relu6 = d.act == F.FD_ACT_RELU6
        assert int(cl[mm // 2, 0]) == 3 and int(cl[0, 0]) == int(cl[1, 0]) == (0 if relu6 else 1) and bool((cl[mm - 1] == 3).all()), (i, cl[:, 0].tolist())
        assert d.act != F.FD_ACT_NONE and 2 not in cl.unique().tolist()
        with np.errstate(invalid="ignore"):
            ref = a32.astype(np.float64) @ w[:, :c].astype(np.float64).T + bias.astype(np.float64)
            ref = np.where(np.isnan(ref), ref, np.minimum(np.maximum(ref, 0.0), 6.0 if relu6 else np.inf))
        assert np.array_equal(_cls(ref).numpy(), cl.numpy()), i
        fin = cl.numpy() == 0
        ex, el = harness.rel_err(outs[0].numpy()[fin], ref[fin]), harness.rel_err(outs[1].numpy()[fin], ref[fin])
        print("X3NONFINITE %s %s layer %d: x3 %.3g fp32-lds %.3g ratio %.2f" % (kind, name, i, ex, el, ex / max(el, 1e-30)))
        assert ex <= 2.0 * el, (i, ex, el)
        worst = max(worst, ex / max(el, 1e-30))
    note(kind, "gemm16_x3_nonfinite_a_rows", name, t0, layers=len(forced), worst_ratio=worst)
    px.close(); pl.close()


def check_nonfinite_classes(kind):
    """Through whole plans: +Inf, -Inf and NaN enter with the image and reach the GEMMs through the layers in front of them (as far as those let them:
    a ReLU6 stage turns +Inf into 6 and -Inf into 0; check_nonfinite_a_rows feeds the GEMM itself).  Every stored tensor and the output have the fp32 form's class
    (finite, +Inf, -Inf, NaN) per element; a producer's planes hold a non-finite value as (a, 0, 0)."""
    t0 = time.time()
    dev = device_of(kind)
    m, x = _model_x(forms.TINY, 2, (64, 64), seed=37)
    _special_weights(m)
    px = harness.CPlan(kind, m, x.to(dev), flags=FORCE)
    pl = harness.CPlan(kind, m, x.to(dev), flags=FP32_LDS)
    assert any(X3_NOTE in s for s in _info(px)) and not any(X3_NOTE in s for s in _info(pl))
    xp = x.clone()
    xp[0, :, 0, 0] = float("inf"); xp[0, :, 32, 32] = float("-inf"); xp[1, :, 0, 63] = float("nan"); xp[1, 0, 31, 31] = float("inf")
    yx, yl = px.forward(xp.to(dev)).cpu(), pl.forward(xp.to(dev)).cpu()
    cls = _cls

    compared = in_planes = 0
    for i in range(len(px.layers)):
        got = _a_planes(px, i)
        if got is not None:
            (hi, mid, lo), f32 = got
            c = f32.shape[1]
            bad = ~np.isfinite(f32)
            assert np.array_equal(_cls(hi[:, :c]).numpy(), _cls(f32).numpy()) and not mid[:, :c][bad].any() and not lo[:, :c][bad].any(), i
            in_planes += int(bad.sum())
        a, b = px.raw(i), pl.raw(i)
        if a is None:
            continue
        ta, tb = torch.from_numpy(a[0].view(np.float32).copy()), torch.from_numpy(b[0].view(np.float32).copy())
        assert torch.equal(cls(ta), cls(tb)), "layer %d: classes differ from the fp32 form's" % i
        fin = torch.isfinite(tb)
        if bool(fin.any()):
            d = float((ta.double() - tb.double())[fin].abs().max()) / max(float(tb[fin].abs().max()), 1e-30)
            assert d < 1e-5, (i, d)
        compared += 1
    assert torch.equal(cls(yx), cls(yl)), "the output's classes differ from the fp32 form's"
    assert bool((~torch.isfinite(yl)).any()) and in_planes > 0
    note(kind, "gemm16_x3_nonfinite", "tiny", t0, tensors=compared, nonfinite_in_planes=in_planes, nonfinite_outputs=int((~torch.isfinite(yl)).sum()))
    px.close(); pl.close()


def check_whole_plan(kind):
    """base_s0 at batch 4, KEEP_ACTIVATIONS, every eligible layer on the form: per-layer and final rel_err against the oracle below TOL = 1e-3, and the final
    one <= 2 x that of the same plan with the form forbidden."""
    from oracle import inputs
    t0 = time.time()
    dev = device_of(kind)
    m, x, _, _ = inputs.golden_case("base_s0")
    x = x[:1].repeat(4, 1, 1, 1) * torch.linspace(0.7, 1.0, 4).view(4, 1, 1, 1)
    e_x, errs, info = harness.compare_with_oracle(kind, m, x, dev, flags=FORCE)       # (at batch 4 only the gemm16 forcing bit gives the form its producers)
    e_f, _, info_f = harness.compare_with_oracle(kind, m, x, dev, flags=F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_NO_G16_X3)
    counts = []
    for flags in (FORCE, F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_NO_G16_X3):        # (compare_with_oracle returns the info lines only: the forms of the same two plans)
        p = harness.CPlan(kind, m, x.to(dev), flags=flags, pack=False)
        counts.append(sum(X3_NOTE in s for s in _info(p)))
        p.close()
    assert counts[0] >= 5 and counts[1] == 0, (counts, info)
    assert max(errs) < 1e-3, errs
    assert e_x <= 2.0 * e_f, (e_x, e_f)
    note(kind, "gemm16_x3_whole_plan", "base_s0_b4", t0, rel_err=e_x, rel_err_fp32_forms=e_f, x3_layers=counts[0])


def _stored_bytes(p, i):
    """layer i's stored tensor as bytes of the workspace (on the plan's device), or None where the plan stores none"""
    ptr, d = ctypes.c_void_p(), [ctypes.c_int32() for _ in range(4)]
    if p.lib.fd_layer_output(p.h, i, ctypes.byref(ptr), *[ctypes.byref(v) for v in d]) != 0:
        return None
    n, h, w, c = [v.value for v in d]
    off = ptr.value - p.ws.data_ptr()
    return p.ws[off:off + n * h * w * c * 4]


def default_and_forced_plans(kind, keep, pack=True):
    from oracle import inputs
    dev = device_of(kind)
    m, x, _, _ = inputs.golden_case("base_s0")
    x = x[:1].repeat(32, 1, 1, 1) * torch.linspace(0.5, 1.0, 32).view(32, 1, 1, 1)
    x = x.to(dev)
    return x, harness.CPlan(kind, m, x, keep=keep, pack=pack), harness.CPlan(kind, m, x, keep=keep, flags=F.FD_TUNE_FORCE_G16_X3, pack=pack)


def same_forms_prefix(pd, pf):
    """-> (layers the default plan runs on the form, n): the first n layers run the same kernel forms in the default and in the forced plan, so their outputs
    depend on identical launches only.  The default batch-32 plan picks conv7.3 ... conv11.3; the forced plan adds later layers (conv12.3 first), so the
    prefix reaches through the depthwise consumer evaluated in conv11.3's epilogue."""
    idd, idf = _info(pd), _info(pf)
    picked = [i for i, s in enumerate(idd) if X3_NOTE in s]
    assert len(picked) == 5 and [pd.layers[i].name for i in picked] == ["conv%d.3" % j for j in range(7, 12)], [pd.layers[i].name for i in picked]
    assert all(X3_NOTE in idf[i] for i in picked) and sum(X3_NOTE in s for s in idf) > 5, idf
    n = 0
    while n < len(idd) and idd[n] == idf[n]:
        n += 1
    assert n >= picked[-1] + 2 and "evaluated in the epilogue" in idd[picked[-1] + 1], (n, picked, idd[picked[-1]:picked[-1] + 3])
    return picked, n


def check_default_plan_is_the_forced_plan_where_it_picks_the_form(kind):
    """batch 32: wherever the pick function chose the same forms as the forcing bit, the default plan equals the forced plan bit for bit.  KEEP_ACTIVATIONS
    plans: every stored tensor of the layers in front of the first layer whose form differs (same_forms_prefix) is compared.  The plans that keep nothing
    pick the same five layers; their outputs differ by the later layers' forms only, within the 2e-6 the project allows between two fp32 kernel choices."""
    t0 = time.time()
    x, pd, pf = default_and_forced_plans(kind, keep=True)
    picked, n = same_forms_prefix(pd, pf)
    pd.forward(x); pf.forward(x)
    compared = 0
    for i in range(n):
        a, b = _stored_bytes(pd, i), _stored_bytes(pf, i)
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b), "layer %d (%s): the default plan differs from the forced plan" % (i, pd.layers[i].name)
            compared += 1
    assert compared >= 20, compared
    pd.close(); pf.close()
    x, pd, pf = default_and_forced_plans(kind, keep=False)
    assert [i for i, s in enumerate(_info(pd)) if X3_NOTE in s] == picked
    yd, yf = pd.forward(x), pf.forward(x)
    e = harness.rel_err(yd.cpu().numpy(), yf.cpu().numpy())
    note(kind, "gemm16_x3_default_vs_forced", "base_s0_b32", t0, picked=len(picked), forced=sum(X3_NOTE in s for s in _info(pf)), same_form_layers=n, bit_equal_tensors=compared, output=e)
    assert e < 2e-6
    pd.close(); pf.close()


def check_default_plan_geometry(kind):
    """the plan-geometry half of the check above (no forward, no weights, an untouched workspace): which layers the default batch-32 plans pick, and how far
    the forced plan agrees -- on the emulator tier too, where the forward of a batch of 32 would take minutes"""
    for keep in (True, False):
        _, pd, pf = default_and_forced_plans(kind, keep=keep, pack=False)
        same_forms_prefix(pd, pf)
        pd.close(); pf.close()
