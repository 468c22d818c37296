"""Non-finite values (NaN, -NaN, +-Inf) through the product's kernels, CPU tier.

The reference propagates them: F.relu / F.hardtanh keep a NaN, a NaN anywhere in a BatchNorm channel makes its batch statistics NaN, and the
backward passes of threshold / hardtanh let the gradient through at a NaN input.  The library must do the same instead of returning a plausible,
finite depth map (or a finite loss for a diverged train step).  Three tiers:
  * the BatchNorm statistics rows (fd_stat_add / fd_stat_total, csrc/fd_device.h) through a ctypes shim, against exact rational sums;
  * emulated inference plans (fp32 / fp16 / bf16, several kernel forms) against oracle/torch_ref.py in fp64: the non-finite mask must be the
    reference's exactly, and the other frames must not notice the poisoned one;
  * emulated train steps (fp32 / bf16, several plan forms) against the fp64 reference: loss, dLoss/dpred, running statistics, gradient pattern,
    and a clean step afterwards that carries nothing of the poisoned one.
"""
import ctypes
import functools
import math
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest
import torch

import harness
from oracle import torch_ref
from test_emu_forward import RAGGED, TINY, small_model

FWD, BWD = 0, 1
# bin boundaries (binary exponents) and fixed-point fractions of fd_stat_fmt
FMT = {FWD: dict(lo=-8, hi=16, frac=(56, 32, 8)), BWD: dict(lo=-32, hi=-8, frac=(80, 56, 32))}


# ---- statistics rows ----------------------------------------------------------------------------------------------------------------

_shim = None


def shim():
    global _shim
    if _shim is None:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
        import build_emu
        L = ctypes.CDLL(build_emu.build_stat_shim())
        P = ctypes.c_void_p
        L.fd_shim_stat_add.argtypes = [ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.c_long, ctypes.c_long]
        L.fd_shim_stat_add.restype = None
        L.fd_shim_stat_total.argtypes = [ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.fd_shim_stat_total.restype = ctypes.c_double
        L.fd_shim_stat_total_sliced.argtypes = [ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.fd_shim_stat_total_sliced.restype = ctypes.c_double
        _shim = L
    return _shim


class Rows:
    """A unit's statistics rows (int64 [nr][3][2][cs], then the poison flags [2][cs]) in host memory."""
    CS = 16

    def __init__(self, nr):
        self.nr = nr
        self.buf = np.zeros((nr * 3 * 2 + 2) * self.CS, np.int64)

    def add(self, d, vals, which=0, c=3, blk0=0):
        v = np.ascontiguousarray(vals, np.float32)
        shim().fd_shim_stat_add(d, self.buf.ctypes.data, self.nr, self.CS, which, c, v.ctypes.data, len(v), blk0)

    def total(self, d, which=0, c=3, RG=1):
        if RG == 1:
            return shim().fd_shim_stat_total(d, self.buf.ctypes.data, self.nr, self.CS, which, c, 0, 1)
        return shim().fd_shim_stat_total_sliced(d, self.buf.ctypes.data, self.nr, self.CS, which, c, RG)


def documented(d, v):
    """The value fd_stat_add documents for the fp32 partial v: exact inside the bins' range, denormals 0, truncated below the lowest
    bin's exact range, the exponent saturated at 47 - frac in the highest bin.  None for Inf / NaN (poison)."""
    v = np.float32(v)
    if not np.isfinite(v):
        return None
    u = int(v.view(np.uint32))
    e = ((u >> 23) & 255) - 127
    if e == -127:
        return Fraction(0)
    f = FMT[d]
    b = 0 if e < f["lo"] else (1 if e < f["hi"] else 2)
    frac = f["frac"][b]
    e = min(e, 47 - frac)
    m = (u & 0x7FFFFF) | 0x800000
    sh = e + frac - 23
    iv = m << sh if sh >= 0 else (m >> -sh if sh > -24 else 0)
    return Fraction(-iv if u >> 31 else iv, 2 ** frac)


def bins_of(d, vals):
    """Exact per-bin totals of the documented values."""
    f = FMT[d]
    out = [Fraction(0)] * 3
    for v in np.asarray(vals, np.float32):
        e = ((int(v.view(np.uint32)) >> 23) & 255) - 127
        b = 0 if e < f["lo"] else (1 if e < f["hi"] else 2)
        out[b] += documented(d, v)
    return out


def check_total(d, vals, got):
    bins = bins_of(d, vals)
    exact = sum(bins)
    if sum(1 for b in bins if b != 0) <= 1:
        assert got == float(exact), (got, float(exact))          # one bin: the exact sum rounded once
    else:                                                          # each bin rounded once, three additions in double
        bound = 4 * 2.0 ** -53 * float(sum(abs(b) for b in bins))
        assert abs(Fraction(got) - exact) <= bound, (got, float(exact), bound)


def boundary_values(d):
    f = FMT[d]
    vals = []
    for e in (f["lo"], f["hi"]):
        x = np.float32(2.0 ** e)
        vals += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))]
    sat = 47 - f["frac"][2]                                        # the highest bin's saturation exponent
    x = np.float32(2.0 ** sat)
    vals += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf)), np.float32(3.0 * 2.0 ** (sat + 5))]
    low = 2.0 ** (-f["frac"][0] + 23)                               # below this the lowest bin truncates
    vals += [np.float32(low), np.float32(low * 0.75), np.float32(1.2345678e-30), np.float32(2.0 ** -126)]
    return [np.float32(v) for v in vals]


@pytest.mark.parametrize("d", [FWD, BWD])
def test_stat_rows_bin_boundaries_and_saturation(d):
    f = FMT[d]
    sat = 47 - f["frac"][2]
    for v in boundary_values(d):
        for s in (1, -1):
            r = Rows(1)
            r.add(d, [s * v])
            check_total(d, [s * v], r.total(d))
            if np.float32(v) < 2.0 ** sat and abs(float(v)) >= 2.0 ** (-f["frac"][0] + 23):
                assert documented(d, s * v) == Fraction(float(s * v))     # inside the documented exact range
    # saturation: a partial at or above 2^sat counts with its exponent clamped to sat
    r = Rows(1)
    r.add(d, [np.float32(1.5 * 2.0 ** (sat + 7))])
    assert r.total(d) == 1.5 * 2.0 ** sat


@pytest.mark.parametrize("d", [FWD, BWD])
def test_stat_rows_denormals_count_as_zero(d):
    den = np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38], np.float32)
    assert all(0 < abs(float(x)) < 2.0 ** -126 for x in den)
    r = Rows(2)
    r.add(d, den)
    assert r.total(d) == 0.0
    r.add(d, [np.float32(0.25), np.float32(-0.0)])
    check_total(d, [np.float32(0.25)], r.total(d))


@pytest.mark.parametrize("d", [FWD, BWD])
@pytest.mark.parametrize("nr", [1, 4, 16])
def test_stat_rows_sign_cancellation(d, nr):
    rng = np.random.default_rng(7 + nr + 10 * d)
    f = FMT[d]
    for scale_e in (f["lo"] - 4, (f["lo"] + f["hi"]) // 2, f["hi"] + 3):
        v = (rng.standard_normal(300) * 2.0 ** scale_e).astype(np.float32)
        vals = np.concatenate([v, -v[::-1]])                        # every partial cancelled by its negation, in another row
        r = Rows(nr)
        r.add(d, vals)
        for RG in (1, 2, 4, 8, 16):
            assert r.total(d, RG=RG) == 0.0
        vals = np.concatenate([vals, np.float32([2.0 ** scale_e, -3 * 2.0 ** (scale_e - 30)])])
        r.add(d, vals[-2:], blk0=len(vals))
        check_total(d, vals, r.total(d))


@pytest.mark.parametrize("d", [FWD, BWD])
@pytest.mark.parametrize("nr", [1, 2, 4, 8, 16])
def test_stat_rows_poison_any_count_any_slicing(d, nr):
    """One to nine non-finite partials, or all of them, in any row: the column's total is NaN in every slicing fd_stat_table_block uses --
    also when the count is a multiple of 4 (an additive 2^62 poison per partial wrapped back to a finite total there)."""
    bad = [np.float32(np.nan), np.float32(-np.nan), np.float32(np.inf), np.float32(-np.inf)]
    rng = np.random.default_rng(nr)
    fin = rng.standard_normal(64).astype(np.float32)
    for k in list(range(1, 10)) + ["all"]:
        n = 64 if k == "all" else k
        for which in (0, 1):
            r = Rows(nr)
            r.add(d, fin, which=which)
            r.add(d, [bad[i % 4] for i in range(n)], which=which, blk0=5)
            for RG in (1, 2, 4, 8, 16):
                assert math.isnan(r.total(d, which=which, RG=RG)), (k, which, RG)
            assert r.total(d, which=1 - which) == 0.0                      # the other sum and ...
            assert r.total(d, which=which, c=4) == 0.0                     # ... the neighbouring column are untouched
            clean = Rows(nr)
            clean.add(d, fin, which=which)
            for RG in (1, 2, 4, 8, 16):
                got = clean.total(d, which=which, RG=RG)
                assert got == clean.total(d, which=which) or abs(got - clean.total(d, which=which)) <= 4e-16 * float(np.abs(fin).sum())


@pytest.mark.parametrize("d", [FWD, BWD])
@pytest.mark.parametrize("b", [0, 1, 2])
def test_stat_rows_headroom_is_exact(d, b):
    """The plan allows FD_STAT_MAX_PARTIALS = 2^15 partials per column over all its rows (fd_train_impl.h headroom check).  Partials just below the
    top of each bin, all of one sign, dealt to 16 rows: the total reaches 2^63 - 2^39 in the bin's integer -- it must still be the exact sum, rounded
    once.  (The plan's earlier limit, 16 rows x 2^14 partials, let the int64 total wrap.)"""
    f = FMT[d]
    top = [f["lo"], f["hi"], 47 - f["frac"][2]][b]
    v = np.nextafter(np.float32(2.0 ** top), np.float32(0))
    n = 2 ** 15
    for s in (1, -1):
        r = Rows(16)
        r.add(d, np.full(n, s * v, np.float32))
        exact = n * Fraction(float(s * v))
        assert documented(d, s * v) == Fraction(float(s * v))
        for RG in (1, 2, 16):
            got = r.total(d, RG=RG)
            if RG == 1:
                assert got == float(exact), (got, float(exact))
            else:
                assert abs(Fraction(got) - exact) <= 2 * 2.0 ** -53 * abs(exact), (RG, got, float(exact))


# ---- inference --------------------------------------------------------------------------------------------------------------------------

NAN_POS = torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)[0].item()
NAN_NEG = torch.tensor([-0x400000], dtype=torch.int32).view(torch.float32)       # 0xFFC00000: a NaN with its sign bit set
POISONS = (("+nan", NAN_POS), ("-nan", None), ("+inf", float("inf")), ("-inf", float("-inf")))
TOLS = {torch.float32: 1e-3, torch.float16: 5e-3, torch.bfloat16: 4e-2}     # the existing forward tests' tolerances against fp32 / fp64 references


def sites(h, w):
    return {"corner": (0, 0), "edge": (0, w // 2 + 1), "centre": (h // 2, w // 2 - 1), "far_corner": (h - 1, w - 1)}


def poisoned_batch(h, w, rot, seed=5):
    """[4 frames with one poisoned pixel (+nan, -nan, +inf, -inf; all three channels), one all-NaN frame, one clean frame] and the clean batch.
    `rot` rotates which site each value goes to, so that the configurations together cover every (value, site) pair."""
    clean = torch.rand(6, 3, h, w, generator=torch.Generator().manual_seed(seed))
    x = clean.clone()
    names = list(sites(h, w))
    where = []
    for f, (pn, val) in enumerate(POISONS):
        site = names[(f + rot) % len(names)]
        yy, xx = sites(h, w)[site]
        if val is None:
            x[f, :, yy, xx] = NAN_NEG[0]          # copies the bits: the sign stays set
            assert int(x[f, 0, yy, xx].view(torch.int32)) == -0x400000
        else:
            x[f, :, yy, xx] = val
        where.append("%s@%s" % (pn, site))
    x[4] = float("nan")
    where += ["all-nan", "clean"]
    return x, clean, where


def reference_forward(model, x):
    p64 = torch_ref.params_from_state(model.state_dict(), torch.float64)
    with torch.no_grad():
        return torch_ref.forward(p64, x.double(), train=False)


def check_nonfinite_forward(y, y_clean, ref, where, tol):
    for f, name in enumerate(where):
        fin_ref, fin = torch.isfinite(ref[f]), torch.isfinite(y[f])
        mism = int((fin_ref != fin).sum())
        assert mism == 0, "frame %d (%s): %d pixels where the non-finite mask differs from the reference's (%d non-finite there, %d here)" % (
            f, name, mism, int((~fin_ref).sum()), int((~fin).sum()))
        assert bool(torch.isnan(y[f]).eq(torch.isnan(ref[f])).all()), (f, name)        # NaN where the reference has NaN, not an infinity
        if bool(fin_ref.any()):
            d = float((y[f].double() - ref[f])[fin_ref].abs().max()) / max(float(ref[f][fin_ref].abs().max()), 1e-30)
            assert d < tol, (f, name, d)
        if "nan" in name and "all" not in name:
            # outside the NaN's footprint nothing changed: bit for bit the clean run
            assert torch.equal(y[f][fin_ref], y_clean[f][fin_ref]), (f, name)
        if name == "clean":
            assert torch.equal(y[f], y_clean[f]), "frame %d: a clean frame behind poisoned ones changed" % f
    assert bool(torch.isfinite(y_clean).all())


F = harness.capi
INFER_CASES = [
    # name, plan, hw, dtype, flags
    ("tiny_f32", TINY, (64, 64), torch.float32, 0),
    ("tiny_f32_rect", TINY, (32, 96), torch.float32, 0),
    ("tiny_f32_gemm16", TINY, (64, 64), torch.float32, F.FD_TUNE_FORCE_GEMM16),
    ("ragged_f32_gemm16_rect", RAGGED, (32, 96), torch.float32, F.FD_TUNE_FORCE_GEMM16),
    ("tiny_f32_units", TINY, (64, 64), torch.float32, F.FD_TUNE_FORCE_UNIT_FUSION),
    ("tiny_f16", TINY, (64, 64), torch.float16, 0),
    ("ragged_f16_rect", RAGGED, (32, 96), torch.float16, 0),
    ("tiny_f16_epi", TINY, (64, 64), torch.float16, F.FD_TUNE_FORCE_EPILOGUE_FUSION),
    ("ragged_f16_gemm16_rect", RAGGED, (32, 96), torch.float16, F.FD_TUNE_FORCE_GEMM16),
    ("tiny_bf16", TINY, (64, 64), torch.bfloat16, 0),
    ("ragged_bf16_rect", RAGGED, (32, 96), torch.bfloat16, 0),
    ("tiny_bf16_epi", TINY, (64, 64), torch.bfloat16, F.FD_TUNE_FORCE_EPILOGUE_FUSION),
    ("ragged_bf16_h8", RAGGED, (64, 64), torch.bfloat16, F.FD_TUNE_FORCE_DW_H8 | F.FD_TUNE_NO_DW5_ROWS),
    ("tiny_bf16_gemm16_rect", TINY, (32, 96), torch.bfloat16, F.FD_TUNE_FORCE_GEMM16),
]


def check_forward_propagates_nonfinite_like_reference(kind, name, plan, hw, dtype, flags):
    """A NaN / -NaN / +-Inf pixel at a corner, an edge or the centre of frame 0 ... 3, an all-NaN frame 4 and a clean frame 5, through an inference
    plan: exactly the reference's non-finite output pixels (no scrubbing by max / med3 / integer ReLU, no halo or padding lane 'masked' by a
    multiplication with 0, which leaves a NaN), the reference's values elsewhere, and the clean frame bit-identical to an all-clean batch.
    kind: "emu" (CPU emulator) or "hip" (the product library on the device)."""
    t0 = time.time()
    dev = torch.device("cpu" if kind == "emu" else "cuda")
    rot = sum(map(ord, name)) % 4
    m = small_model(plan[0], plan[1], seed=17).eval()
    x, clean, where = poisoned_batch(hw[0], hw[1], rot)
    ref = reference_forward(m, x)[:, 0]
    p = harness.CPlan(kind, m, x.to(dev), keep=False, dtype=dtype, flags=flags)
    try:
        y = p.forward(x.to(dev))[:, 0].cpu()
        y_clean = p.forward(clean.to(dev))[:, 0].cpu()
        info = p.info()
    finally:
        p.close()
    if flags == F.FD_TUNE_FORCE_GEMM16:
        assert sum(s.startswith("pw_gemm16") for s in info) == 18, info
    if flags == F.FD_TUNE_FORCE_UNIT_FUSION:
        assert any(s.startswith("dwpw<") for s in info), info
    if flags == F.FD_TUNE_FORCE_EPILOGUE_FUSION:
        assert any("evaluated in the epilogue" in s for s in info), info
    if dtype != torch.float32 and flags == 0 and plan is RAGGED:
        assert any(s.startswith("dw5_rows<") for s in info), info          # the packed-pair 5x5 kernel and its packed ReLU
    fin = torch.isfinite(ref)
    print("FORMS %s forward_propagates_nonfinite[%s] finite_pixels_rel_err=%.3g tol=%g nonfinite_mask_mismatches=%d" % (
        kind, name, float((y.double() - ref)[fin].abs().max()) / float(ref[fin].abs().max()), TOLS[dtype], int((torch.isfinite(y) != fin).sum())), end="")
    check_nonfinite_forward(y, y_clean, ref, where, TOLS[dtype])
    print(" wall=%.2fs" % (time.time() - t0))


@pytest.mark.parametrize("name,plan,hw,dtype,flags", INFER_CASES, ids=[c[0] for c in INFER_CASES])
def test_emulated_forward_propagates_nonfinite_like_reference(name, plan, hw, dtype, flags):
    check_forward_propagates_nonfinite_like_reference("emu", name, plan, hw, dtype, flags)


# ---- train step -------------------------------------------------------------------------------------------------------------------------

def library_l1(lib, pred, target):
    """The library's L1 loss kernel (fd_l1_loss): loss and dLoss/dpred."""
    dpred, loss = torch.empty_like(pred), torch.zeros(1, device=pred.device)
    scratch = torch.empty(lib.fd_l1_loss_scratch_bytes(pred.numel()), dtype=torch.uint8, device=pred.device)
    harness.capi.check(lib, lib.fd_l1_loss(pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), loss.data_ptr(), pred.numel(), scratch.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream if pred.is_cuda else None), "fd_l1_loss")
    if pred.is_cuda:
        torch.cuda.synchronize()
    return float(loss), dpred


def reference_train_step(model, x, target):
    """fp64 reference of one train step: prediction, loss, dLoss/dpred, updated running statistics, gradients."""
    from oracle import oracle
    p = torch_ref.params_from_state(model.state_dict(), torch.float64, requires_grad=True)
    pred = torch_ref.forward(p, x.double(), train=True)
    pred.retain_grad()
    loss = (pred - target.double()).abs().mean()
    # (one thread for the backward: torch's CPU hardtanh_backward blocks the gradient at a NaN input in its vectorised body but passes it in the
    # scalar tail of every per-thread chunk, so with several threads the encoder's pattern would depend on the chunking; fd_actgate blocks it)
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        loss.backward()
    finally:
        torch.set_num_threads(nt)
    names = oracle.unit_names()
    grads = {}
    for cp, bp, _, _, _ in names:
        for k in (cp + ".weight", bp + ".weight", bp + ".bias"):
            grads[k] = p[k].grad.detach()
    running = {bp: (p[bp + ".running_mean"].detach(), p[bp + ".running_var"].detach()) for _, bp, _, _, _ in names}
    return pred.detach(), float(loss.detach()), pred.grad.detach(), running, grads


class TrainStep:
    """One train step on a CTrainPlan (parameters, running statistics and num_batches_tracked restorable)."""

    def __init__(self, kind, model, x, dtype, flags):
        self.tp = harness.CTrainPlan(kind, model, x, dtype=dtype, flags=flags)
        self.init = [{k: v.clone() for k, v in d.items()} for d in self.tp.tensors]
        self.nbt = torch.zeros(self.tp.n, dtype=torch.int64, device=x.device)
        for i, q in enumerate(self.tp.params):
            q.bn_num_batches_tracked = self.nbt[i:i + 1].data_ptr()

    def restore(self):
        for d, d0 in zip(self.tp.tensors, self.init):
            for k in d:
                d[k].copy_(d0[k])
        self.nbt.zero_()

    def run(self, x, target):
        y = self.tp.forward(x)
        loss, dpred = library_l1(self.tp.lib, y, target.to(y.device))
        grads = self.tp.backward(dpred)
        names = [l.name for l in self.tp.layers]
        out = {"pred": y.cpu(), "loss": loss, "dpred": dpred.cpu(), "nbt": self.nbt.cpu().clone(), "grads": {}, "running": {}}
        from oracle import oracle
        for (cp, bp, _, _, _), g, d in zip(oracle.unit_names(), grads, self.tp.tensors):
            out["grads"][cp + ".weight"] = g["conv_weight"].cpu().clone()
            out["grads"][bp + ".weight"] = g["bn_weight"].cpu().clone()
            out["grads"][bp + ".bias"] = g["bn_bias"].cpu().clone()
            out["running"][bp] = (d["bn_mean"].cpu().clone(), d["bn_var"].cpu().clone())
        return out

    def close(self):
        self.tp.close()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_nonfinite_train_step(got, ref):
    pred_r, loss_r, dpred_r, running_r, grads_r = ref
    assert math.isnan(loss_r) and not math.isfinite(got["loss"]), got["loss"]
    assert torch.equal(torch.isfinite(got["pred"]), torch.isfinite(pred_r)), "prediction: non-finite pattern differs from the reference's"
    assert torch.equal(got["dpred"].double(), dpred_r), "dLoss/dpred differs from torch's (sign(NaN) = 0)"
    for bp, (rm_r, rv_r) in running_r.items():
        rm, rv = got["running"][bp]
        assert torch.equal(torch.isfinite(rm), torch.isfinite(rm_r)), (bp, "running_mean")
        assert torch.equal(torch.isfinite(rv), torch.isfinite(rv_r)), (bp, "running_var")
    assert bool((got["nbt"] == 1).all()), got["nbt"]
    bad_ref = {k for k, g in grads_r.items() if not bool(torch.isfinite(g).all())}
    bad = {k for k, g in got["grads"].items() if not bool(torch.isfinite(g).all())}
    assert bad == bad_ref, "gradient tensors with a non-finite entry: only here %s, only in the reference %s" % (sorted(bad - bad_ref), sorted(bad_ref - bad))
    return len(bad), len(grads_r)


def check_clean_step_after_poison(kind, model, x, target, dtype, flags, step):
    """The poisoned plan, parameters and running statistics restored, takes a clean step: bit for bit the clean step of a fresh plan."""
    step.restore()
    again = step.run(x, target)
    fresh = TrainStep(kind, model, x, dtype, flags)
    want = fresh.run(x, target)
    fresh.close()
    assert math.isfinite(want["loss"]) and again["loss"] == want["loss"]
    for key in ("pred", "dpred"):
        assert same_bits(again[key], want[key]), key
    for k in want["grads"]:
        assert same_bits(again["grads"][k], want["grads"][k]), k
    for bp in want["running"]:
        assert same_bits(again["running"][bp][0], want["running"][bp][0]) and same_bits(again["running"][bp][1], want["running"][bp][1]), bp
    assert torch.equal(again["nbt"], want["nbt"])


TRAIN_CASES = [
    ("f32", torch.float32, 0),
    ("f32_no_consumer_finalize", torch.float32, F.FD_TUNE_NO_CONSUMER_FINALIZE),
    ("f32_dw_bwd1", torch.float32, F.FD_TUNE_DW_BWD1),
    ("f32_no_bwd_pairing", torch.float32, F.FD_PLAN_NO_BWD_PAIRING),
    ("bf16", torch.bfloat16, 0),
    ("bf16_no_consumer_finalize", torch.bfloat16, F.FD_TUNE_NO_CONSUMER_FINALIZE),
    ("bf16_dw_bwd1", torch.bfloat16, F.FD_TUNE_DW_BWD1),
    ("bf16_no_bwd_pairing", torch.bfloat16, F.FD_PLAN_NO_BWD_PAIRING),
]


@functools.lru_cache(maxsize=None)
def nan_pixel_step_case():
    """(module, clean x, target, x with a NaN pixel in frame 0, fp64 reference of the poisoned step): computed once, shared by the cases of both
    tiers, never modified (a TrainStep works on private copies of the parameters)."""
    m = small_model(TINY[0], TINY[1], seed=3).train()
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 64, 64, generator=g)
    target = 2.0 + torch.rand(2, 1, 64, 64, generator=g)
    xp = x.clone()
    xp[0, :, 21, 40] = float("nan")
    return m, x, target, xp, reference_train_step(m, xp, target)


def check_train_step_with_nan_pixel_like_reference(kind, name, dtype, flags):
    """A NaN pixel in frame 0 of a train step: the batch statistics of the stem are NaN, so -- as in the reference -- every later unit's are,
    the prediction and the loss are NaN, dLoss/dpred is torch's sign(NaN) = 0, num_batches_tracked still counts the step, and the same set of
    gradient tensors carries a non-finite entry.  Nothing of it survives into the next (clean) step of the same plan.
    kind: "emu" (CPU emulator) or "hip" (the product library on the device)."""
    t0 = time.time()
    dev = torch.device("cpu" if kind == "emu" else "cuda")
    m, x, target, xp, ref = nan_pixel_step_case()
    step = TrainStep(kind, m, xp.to(dev), dtype, flags)
    try:
        got = step.run(xp.to(dev), target)
        n_bad, n = check_nonfinite_train_step(got, ref)
        print("FORMS %s train_step_with_nan_pixel[%s] gradient_tensors_with_nonfinite=%d/%d (the reference's set exactly)" % (kind, name, n_bad, n), end="")
        assert n == 114 and n_bad > 0
        if flags == 0:                     # (the clean step afterwards: once per storage type)
            check_clean_step_after_poison(kind, m, x.to(dev), target, dtype, flags, step)
        print(" wall=%.2fs (the shared fp64 reference is computed by the first case)" % (time.time() - t0))
    finally:
        step.close()


@pytest.mark.parametrize("name,dtype,flags", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_emulated_train_step_with_nan_pixel_like_reference(name, dtype, flags):
    check_train_step_with_nan_pixel_like_reference("emu", name, dtype, flags)
