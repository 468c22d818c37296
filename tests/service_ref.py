"""Edge-case checks of the service kernels around the network: fd_l1_loss, fd_l1_loss_masked, fd_sgd_step, fd_cast_gradients, fd_depth_metrics and
fd_depth_metrics_frames, through the public C ABI only.  TEST INFRASTRUCTURE ONLY: shared by the CPU tier (tests/test_service.py: kind = "emu", the
kernels compiled with -DFD_EMU on CPU tensors) and the GPU tier (tests/test_gpu_service.py: kind = "hip", the product library on an MI355X).  Same case
tables, seeds, bounds and assertions in both; the device follows from `kind`.

Every reference is plain numpy / torch on the CPU in fp64, or integer arithmetic for the casts.  Every buffer a kernel writes (dpred, loss, scratch, params,
momentum, the cast destination, sums) is a view into a larger allocation (`Arena`) with at least 8 guard elements of a fixed bit pattern before and after it:
the guards must be bit-identical afterwards, and so must the read-only inputs.  The data regions start out as that pattern too (a NaN in every float type), so
an element a kernel never wrote cannot pass for a result."""
import functools
import math
import time

import numpy as np
import torch

import forms
import harness
from fastdepth_hip import capi

INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
PATTERN = {1: 0xA5, 2: 0x7FA5, 4: 0x7FA5C3A5, 8: 0x7FF5A5A5C3C3A5A5}      # a (signalling) NaN in bf16 / fp32 / fp64
U = 2.0 ** -24                                                            # fp32 unit roundoff


def _stream(kind):
    return torch.cuda.current_stream().cuda_stream if kind == "hip" else None


def _bits(t):
    """CPU integer view of a tensor's bits (numpy)."""
    return t.contiguous().view(INT[t.element_size()]).cpu().numpy()


class Arena:
    """One allocation filled with PATTERN; `sizes[i]` elements of `dtype` are carved out of it so that view i starts `shift[i]` elements behind a 16-byte
    boundary, with at least `guard` pattern elements before, between and after the views."""

    def __init__(self, kind, dtype, sizes, shift=0):
        dev = forms.device_of(kind)
        self.dtype = dtype
        self.item = item = torch.empty((), dtype=dtype).element_size()
        self.guard = guard = max(8, 64 // item)
        per16 = max(16 // item, 1)
        shifts = [shift] * len(sizes) if isinstance(shift, int) else list(shift)
        raw = torch.empty(sum(sizes) + len(sizes) * (guard + per16 + max(shifts)) + guard, dtype=INT[item], device=dev)
        mis = (raw.data_ptr() % 16) // item
        pos, self.offs = 0, []
        for n, s in zip(sizes, shifts):
            pos += guard
            pos += (-(mis + pos)) % per16
            pos += s
            self.offs.append(pos)
            pos += n
        pos += guard
        self.raw = raw[:pos]
        self.raw.fill_(PATTERN[item])
        self.sizes = list(sizes)
        mask = torch.ones(pos, dtype=torch.bool)
        for o, n in zip(self.offs, sizes):
            mask[o:o + n] = False
        self.gmask = mask.to(dev)
        self.dmask = ~self.gmask

    def view(self, i=0):
        o = self.offs[i]
        return self.raw[o:o + self.sizes[i]].view(self.dtype)

    def ptr(self, i=0):
        return self.raw.data_ptr() + self.offs[i] * self.item

    def load(self, flat):
        """the views, in order, <- consecutive pieces of the flat CPU tensor `flat`"""
        self.raw[self.dmask] = flat.contiguous().view(INT[self.item]).to(self.raw.device)

    def data(self):
        """all views concatenated, on the CPU"""
        return self.raw[self.dmask].cpu().view(self.dtype)

    def bad_guards(self):
        return int((self.raw[self.gmask] != PATTERN[self.item]).sum())


def _nan_scratch(kind, nbytes):
    a = Arena(kind, torch.uint8, [nbytes])
    a.view().fill_(0xFF)                                                   # every float / double of it a NaN
    return a


# ---- fd_l1_loss / fd_l1_loss_masked -----------------------------------------------------------------------------------------------------

L1_SIZES = [1, 63, 64, 255, 256, 257, 1000, 16385, 262144, 262401, 600001]     # 16 385: 65 first-stage blocks; the last two wrap the 1024-block grid
L1_WRAP_SIZES = (262401, 600001)
L1_MASKED_SPECIALS = [("none_valid", 257), ("none_valid", 16385), ("single_valid", 257), ("single_valid", 16385), ("nan_pred", 257), ("nan_pred", 16385)]
L1_LOSS_REL = 2.0 ** -18     # non-negative terms, fewer than 64 fp32 roundings: <= 3 per work-item, 6 shuffle levels, 3 wave adds, the finisher


@functools.lru_cache(maxsize=None)
def l1_case(numel, variant):
    """(pred, target) on the CPU, computed once and never modified.  variant: "plain" (unmasked form), "mixed", "none_valid", "single_valid", "nan_pred"."""
    g = torch.Generator().manual_seed(7 * numel + 1)
    pred, target = torch.rand(numel, generator=g) * 10, torch.rand(numel, generator=g) * 10
    i = torch.arange(numel)
    tie = i % 7 == 3
    pred[tie] = target[tie]                                                # exact ties
    nz = i % 11 == 5
    pred[nz], target[nz] = -0.0, 0.0                                       # pred - target = -0.0
    pz = i % 11 == 6
    pred[pz], target[pz] = 0.0, -0.0
    if variant != "plain":
        target[i % 5 == 1] = 0.0
        neg = i % 13 == 2
        target[neg] = -target[neg] - 0.25
        target[i % 17 == 4] = float("nan")
    pred[-1], target[-1] = 9.0, 0.5                                        # the last element (alone in the last block at 256 k + 1) is valid and weighs |d| = 8.5
    if variant in ("none_valid", "single_valid"):
        bad = torch.tensor([0.0, -1.5, float("nan"), -0.0])[i % 4]
        keep = torch.zeros(numel, dtype=torch.bool)
        if variant == "single_valid":
            keep[numel // 2] = True
            pred[numel // 2], target[numel // 2] = 2.5, 4.0
        target = torch.where(keep, target, bad)
    if variant == "nan_pred":
        k = int(torch.nonzero(target > 0)[0])
        pred[k] = float("nan")
    return pred, target


def _l1_call(kind, masked, pred, target, scratch=None):
    L = harness.get_lib(kind)
    dev = forms.device_of(kind)
    numel = pred.numel()
    pd, td = pred.to(dev), target.to(dev)
    dpred, loss = Arena(kind, torch.float32, [numel]), Arena(kind, torch.float32, [1])
    scratch = scratch or _nan_scratch(kind, L.fd_l1_loss_scratch_bytes(numel))
    fn = L.fd_l1_loss_masked if masked else L.fd_l1_loss
    capi.check(L, fn(pd.data_ptr(), td.data_ptr(), dpred.ptr(), loss.ptr(), numel, scratch.ptr(), _stream(kind)), "fd_l1_loss")
    return {"dpred": _bits(dpred.view()), "loss": _bits(loss.view()), "guards": dpred.bad_guards() + loss.bad_guards() + scratch.bad_guards(),
            "inputs_changed": int(not (np.array_equal(_bits(pd), _bits(pred)) and np.array_equal(_bits(td), _bits(target))))}


def check_l1(kind, masked, numel, variant):
    t0 = time.time()
    pred, target = l1_case(numel, variant)
    r, r2 = _l1_call(kind, masked, pred, target), _l1_call(kind, masked, pred, target)
    p64, t64 = pred.numpy().astype(np.float64), target.numpy().astype(np.float64)
    valid = t64 > 0 if masked else np.ones(numel, dtype=bool)
    count = int(valid.sum())
    d = p64 - t64
    with np.errstate(invalid="ignore"):
        ref = np.abs(d[valid]).sum() / count if count else float("nan")
        want_sign = np.where(valid & ~np.isnan(d), np.sign(d), 0.0)
    dp = r["dpred"].view(np.float32)
    loss = float(r["loss"].view(np.float32)[0])
    nzero = want_sign != 0
    mags = np.unique(r["dpred"][nzero] & 0x7FFFFFFF)
    mag = float(mags.view(np.float32)[0]) if mags.size else float("nan")
    inv_ref = 1.0 / count if count else float("nan")
    ulp = float(np.spacing(np.float32(inv_ref))) if count else float("nan")
    implied = int(round(1.0 / mag)) if mags.size == 1 and mag > 0 else -1
    loss_dev = abs(loss - ref) / ref if ref == ref else float(not math.isnan(loss))
    forms.note(kind, "l1_masked" if masked else "l1", "%s-%d" % (variant, numel), t0, loss=loss, ref=float(ref), loss_rel_dev=float(loss_dev), loss_bound=L1_LOSS_REL,
               count=count, implied_count=implied, magnitudes=int(mags.size), mag_dev_ulp=(abs(mag - inv_ref) / ulp if mags.size else 0.0),
               guards_touched=r["guards"] + r2["guards"], inputs_changed=r["inputs_changed"])
    assert r["guards"] == 0 and r2["guards"] == 0 and not r["inputs_changed"] and not r2["inputs_changed"]
    assert np.array_equal(r["dpred"], r2["dpred"]) and np.array_equal(r["loss"], r2["loss"]), "two calls on the same inputs differ"
    assert np.all(dp[~nzero] == 0.0), "non-zero gradient on a tie / an invalid pixel"
    if nzero.any():
        assert mags.size == 1, "the non-zero gradient magnitudes are not one bit pattern: %s" % mags[:4]
        assert np.array_equal(np.sign(dp[nzero]), want_sign[nzero])
        assert abs(mag - inv_ref) <= ulp
        assert implied == count
    if ref == ref:
        assert abs(loss - ref) <= L1_LOSS_REL * ref
    else:
        assert math.isnan(loss)


def check_l1_scratch_reuse(kind, masked):
    """A call at 600 001 (1024 partials) and then one at 257 (2 partials) on the same scratch: bit for bit the 257 call on fresh, NaN-filled scratch."""
    t0 = time.time()
    L = harness.get_lib(kind)
    variant = "mixed" if masked else "plain"
    scratch = _nan_scratch(kind, L.fd_l1_loss_scratch_bytes(600001))
    _l1_call(kind, masked, *l1_case(600001, variant), scratch=scratch)
    reused = _l1_call(kind, masked, *l1_case(257, variant), scratch=scratch)
    fresh = _l1_call(kind, masked, *l1_case(257, variant))
    same = np.array_equal(reused["loss"], fresh["loss"]) and np.array_equal(reused["dpred"], fresh["dpred"])
    forms.note(kind, "l1_scratch_reuse", "masked" if masked else "plain", t0, bit_equal=int(same), guards_touched=reused["guards"] + fresh["guards"])
    assert same and reused["guards"] == 0 and fresh["guards"] == 0


# ---- fd_sgd_step ------------------------------------------------------------------------------------------------------------------------

SGD_NUMELS = [1, 2, 3, 4, 5, 7, 8, 31, 255, 256, 257, 1023, 1024, 1025, 65536, 65537, 70003, 131075]
SGD_SIZES = [SGD_NUMELS[i % len(SGD_NUMELS)] for i in range(130)]          # gridDim.y = 130 > the product's 114 tensors
SGD_LAYOUTS = [("aligned", (0, 0, 0)), ("param_off1", (1, 0, 0)), ("grad_off2", (0, 2, 0)), ("mom_off3", (0, 0, 3)), ("all_off1", (1, 1, 1))]   # elements behind 16 bytes: (param, grad, momentum)
SGD_HYPER = [(0.01, 0.9, 1e-4, 1.0), (0.01, 0.9, 1e-4, 0.5), (0.1, 0.0, 0.0, 1.0), (0.01, 0.9, 0.0, 1.0)]     # (lr, momentum, wd, grad_scale)


@functools.lru_cache(maxsize=None)
def sgd_data():
    """(params, three gradient sets), flat, on the CPU: computed once, never modified."""
    g = torch.Generator().manual_seed(11)
    n = sum(SGD_SIZES)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(3)]


class _SgdState:
    def __init__(self, kind, shifts):
        self.kind, self.L = kind, harness.get_lib(kind)
        self.P, self.G, self.M = [Arena(kind, torch.float32, SGD_SIZES, s) for s in shifts]
        self.P.load(sgd_data()[0])
        self.M.load(torch.full((sum(SGD_SIZES),), float("nan")))
        rec = []
        for i, n in enumerate(SGD_SIZES):
            rec += [self.P.ptr(i), self.G.ptr(i), self.M.ptr(i), n]
        self.table = torch.tensor(rec, dtype=torch.int64).to(forms.device_of(kind))       # as TrainEngine builds it

    def step(self, grads, hyper, first):
        self.G.load(grads)
        before = self.G.raw.clone()
        lr, mom, wd, gs = hyper
        capi.check(self.L, self.L.fd_sgd_step(self.table.data_ptr(), len(SGD_SIZES), sum(SGD_SIZES), lr, mom, wd, gs, int(first), _stream(self.kind)), "fd_sgd_step")
        return self.P.bad_guards() + self.M.bad_guards(), int(not torch.equal(before, self.G.raw))


def check_sgd(kind, layout, shifts, hyper):
    t0 = time.time()
    st = _SgdState(kind, shifts)
    lr, mom, wd, gs = [float(np.float32(v)) for v in hyper]               # the C ABI takes floats: these are the fp32 inputs of the update
    _, grads = sgd_data()
    p = st.P.data().numpy().astype(np.float64)
    m = np.zeros_like(p)
    worst_m = worst_p = 0.0
    for step in (0, 1):
        guards, grads_changed = st.step(grads[step], hyper, first=step == 0)
        g = grads[step].numpy().astype(np.float64)
        d = wd * p + gs * g
        m_ref = d if step == 0 else mom * m + d
        p_ref = p - lr * m_ref
        S = np.abs(wd * p) + np.abs(gs * g) + (0.0 if step == 0 else np.abs(mom * m))
        m_got, p_got = st.M.data().numpy().astype(np.float64), st.P.data().numpy().astype(np.float64)
        nan_left = int(np.isnan(m_got).sum() + np.isnan(p_got).sum())
        m_bound = 4 * U * S
        p_bound = 2 * U * (np.abs(p) + lr * np.abs(m_ref)) + 4 * U * lr * S
        with np.errstate(invalid="ignore", divide="ignore"):
            rm, rp = np.abs(m_got - m_ref) / m_bound, np.abs(p_got - p_ref) / p_bound
        rm[(m_got == m_ref) & (m_bound == 0)] = 0.0
        wm, wp = float(np.nan_to_num(rm, nan=np.inf).max()), float(np.nan_to_num(rp, nan=np.inf).max())
        worst_m, worst_p = max(worst_m, wm), max(worst_p, wp)
        forms.note(kind, "sgd", "%s-lr%g-m%g-wd%g-gs%g-step%d" % ((layout,) + tuple(hyper) + (step,)), t0, m_err_over_bound=wm, p_err_over_bound=wp, nan_left=nan_left,
                   guards_touched=guards, grads_changed=grads_changed)
        assert guards == 0 and not grads_changed
        assert nan_left == 0, "first_step must not read the momentum buffer" if step == 0 else "NaN after the second step"
        assert wm <= 1.0, int(np.argmax(np.nan_to_num(rm, nan=np.inf)))
        assert wp <= 1.0, int(np.argmax(np.nan_to_num(rp, nan=np.inf)))
        p, m = p_got, m_got                                              # the next step's fp32 inputs
    return worst_m, worst_p


def check_sgd_against_torch(kind):
    """Three steps of the all-aligned layout against torch.optim.SGD."""
    t0 = time.time()
    st = _SgdState(kind, (0, 0, 0))
    p0, grads = sgd_data()
    ref = [q.clone().requires_grad_(True) for q in p0.split(SGD_SIZES)]
    opt = torch.optim.SGD(ref, lr=0.01, momentum=0.9, weight_decay=1e-4)
    for step in range(3):
        for q, gr in zip(ref, grads[step].split(SGD_SIZES)):
            q.grad = gr.clone()
        opt.step()
        guards, grads_changed = st.step(grads[step], (0.01, 0.9, 1e-4, 1.0), first=step == 0)
        assert guards == 0 and not grads_changed
    got, want = st.P.data(), torch.cat([q.detach() for q in ref])
    forms.note(kind, "sgd_against_torch", "aligned-3steps", t0, max_abs_dev=float((got - want).abs().max()), rtol=1e-6)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)


# ---- fd_cast_gradients ------------------------------------------------------------------------------------------------------------------

CAST_LAYOUTS = [("packed", (0, 0)), ("f32_off1", (1, 0)), ("bf16_off1", (0, 1)), ("mixed_bf16_at_8_mod_16", (0, 4))]      # elements behind 16 bytes: (fp32 side, bf16 side)
CAST_VALUE_CASES = [(name, sh, 0) for name, sh in CAST_LAYOUTS] + [("packed", (0, 0), 1), ("packed", (0, 0), 2), ("packed", (0, 0), 3)]     # (layout, shifts, tail)
CAST_SIZE_CASES = [(n, 0) for n in (1, 2, 3, 4, 5, 1023, 1025, 2098181)] + [(2098181, 1)]      # 2 098 181 = one wrap of the 2048-block grid + 1029; (numel, source shift)


@functools.lru_cache(maxsize=None)
def cast_f32_set():
    """Every upper half x six lower halves, shuffled with a fixed seed (uint32, 393 216 values): +-0, subnormals, ties to even both ways, overflow to +-Inf,
    +-Inf, quiet and signalling NaNs of both signs, every class in every lane position of the packed form."""
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    u = ((np.arange(65536, dtype=np.uint32) << 16)[None, :] | lows[:, None]).reshape(-1)
    np.random.default_rng(7).shuffle(u)
    return u


@functools.lru_cache(maxsize=None)
def cast_bf16_set():
    u = np.arange(65536, dtype=np.uint16)
    np.random.default_rng(8).shuffle(u)
    return u


def bf16_rule(u):
    """fd_device.h's documented fp32 -> bf16 conversion on the bits: round to nearest even, a NaN keeps its sign and upper payload and is quieted."""
    u = u.astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16), nan


def _cast(kind, src_bits, to_bf16, shifts):
    """src_bits (numpy uint32 / uint16) through fd_cast_gradients; -> (destination bits, guard elements touched, source changed)"""
    L = harness.get_lib(kind)
    n = src_bits.size
    f32, b16 = Arena(kind, torch.float32, [n], shifts[0]), Arena(kind, torch.bfloat16, [n], shifts[1])
    src, dst = (f32, b16) if to_bf16 else (b16, f32)
    src.load(torch.from_numpy(src_bits.view(np.int32 if to_bf16 else np.int16).copy()))
    assert (src.ptr() % 16, dst.ptr() % 16) == ((4 * shifts[0]) % 16, (2 * shifts[1]) % 16)[::1 if to_bf16 else -1]
    capi.check(L, L.fd_cast_gradients(src.ptr(), dst.ptr(), n, int(to_bf16), _stream(kind)), "fd_cast_gradients")
    got = _bits(dst.view()).view(np.uint16 if to_bf16 else np.uint32)
    changed = int(not np.array_equal(_bits(src.view()).view(src_bits.dtype), src_bits)) + src.bad_guards()
    return got, dst.bad_guards(), changed


def _with_tail(u, tail):
    return np.concatenate([u, u[:tail]]) if tail else u


def check_cast_to_bf16_values(kind, layout, shifts, tail):
    t0 = time.time()
    u = _with_tail(cast_f32_set(), tail)
    got, guards, changed = _cast(kind, u, True, shifts)
    want, nan = bf16_rule(u)
    sub = ~nan & ((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)
    ne = got != want
    torch_bits = torch.from_numpy(u.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan_kept = ((got[nan] & 0x7FFF) > 0x7F80) & ((got[nan] >> 15) == (u[nan] >> 31))
    forms.note(kind, "cast_f32_to_bf16_values", "%s-tail%d" % (layout, tail), t0, values=int(u.size), nan_inputs=int(nan.sum()), nan_not_kept=int((~nan_kept).sum()),
               nan_payload_mismatch=int(ne[nan].sum()), subnormal_mismatch=int(ne[sub].sum()), other_mismatch=int(ne[~nan & ~sub].sum()),
               torch_mismatch=int((got[~nan] != torch_bits[~nan]).sum()), guards_touched=guards, source_changed=changed)
    assert guards == 0 and not changed
    assert not ne[~nan].any(), "first mismatch: input %#x -> %#x, rule %#x" % (u[~nan][ne[~nan]][0], got[~nan][ne[~nan]][0], want[~nan][ne[~nan]][0])
    assert np.array_equal(got[~nan], torch_bits[~nan])
    assert nan_kept.all(), "a NaN did not stay a NaN of its sign"
    assert not ne[nan].any(), "NaN payload: input %#x -> %#x, rule %#x" % (u[nan][ne[nan]][0], got[nan][ne[nan]][0], want[nan][ne[nan]][0])


def check_cast_from_bf16_values(kind, layout, shifts, tail):
    t0 = time.time()
    b = _with_tail(cast_bf16_set(), tail)
    got, guards, changed = _cast(kind, b, False, shifts)
    bad = int((got != (b.astype(np.uint32) << 16)).sum())
    forms.note(kind, "cast_bf16_to_f32_values", "%s-tail%d" % (layout, tail), t0, values=int(b.size), mismatch=bad, guards_touched=guards, source_changed=changed)
    assert guards == 0 and not changed and bad == 0


def check_cast_sizes(kind, numel, src_shift):
    """Random gradients (and random bf16 patterns) at `numel`, both directions, then the round trip against torch's own bfloat16 rounding."""
    t0 = time.time()
    x = torch.randn(numel, generator=torch.Generator().manual_seed(numel % 1000 + 3)) * 0.03
    u = x.view(torch.int32).numpy().view(np.uint32)
    got, guards, changed = _cast(kind, u, True, (src_shift, 0))
    bad_to = int((got != bf16_rule(u)[0]).sum())
    back, guards2, changed2 = _cast(kind, got, False, (0, src_shift))
    bad_from = int((back != (got.astype(np.uint32) << 16)).sum())
    want = x.bfloat16().float().view(torch.int32).numpy().view(np.uint32)
    bad_trip = int((back != want).sum())
    forms.note(kind, "cast_sizes", "%d-src_off%d" % (numel, src_shift), t0, to_bf16_mismatch=bad_to, to_f32_mismatch=bad_from, round_trip_mismatch=bad_trip,
               guards_touched=guards + guards2, source_changed=changed + changed2)
    assert guards == 0 and guards2 == 0 and not changed and not changed2
    assert bad_to == 0 and bad_from == 0 and bad_trip == 0


# ---- fd_depth_metrics / fd_depth_metrics_frames -----------------------------------------------------------------------------------------

COUNT_SUMS = (0, 5, 6, 7)
REAL_SUMS = (1, 2, 3, 4, 8, 9)
THRESHOLDS = (1.25, 1.5625, 1.953125)
NEAR = 2.0 ** -20
# (n_frames, frame_numel, seed): the seeds are the first ones (from 1) at which no fp64 ratio lies within 2^-20 relative of a threshold (asserted in every case)
METRICS_POOLED = [(1, 1, 1), (1, 255, 1), (1, 257, 1), (1, 16385, 1), (1, 262401, 1)]
METRICS_FRAMES = [(1, 1, 1), (3, 777, 1), (65, 257, 1), (2, 16641, 1)]       # 16 641 wraps the 64 blocks of a frame
METRICS_SPECIALS = ["target_zero", "output_zero", "output_negative", "both_nonpositive", "output_nan"]


def metrics_elements(out, tgt, dt):
    """The ten per-pixel terms of oracle/metrics.py (row k = the terms of sum k) over the valid pixels, every operation carried out in `dt`."""
    out, tgt = np.asarray(out, np.float32).reshape(-1), np.asarray(tgt, np.float32).reshape(-1)
    valid = (tgt > 0) | (out > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o, t = dt(1e3) * out[valid].astype(dt), dt(1e3) * tgt[valid].astype(dt)
        ad = np.abs(o - t)
        c = dt(math.log(10))
        ratio = np.maximum(o / t, t / o)
        inv = np.abs(dt(1) / o - dt(1) / t)
        e = np.stack([np.ones_like(ad), ad * ad, ad, np.abs(np.log(o) / c - np.log(t) / c), ad / t] + [(ratio < th).astype(dt) for th in THRESHOLDS] + [inv * inv, inv])
    assert e.dtype == dt
    return e, ratio


def metrics_reference(out, tgt):
    """(ten fp64 sums, their budgets, share of pixels whose fp64 ratio is within 2^-20 relative of a threshold without being on it)"""
    e64, ratio = metrics_elements(out, tgt, np.float64)
    e32, _ = metrics_elements(out, tgt, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sums = e64.sum(axis=1)
        diff = np.abs(e32.astype(np.float64) - e64)
        diff[~np.isfinite(diff)] = 0.0
        mag = np.abs(e64)
        mag[~np.isfinite(mag)] = 0.0
        budget = 4 * diff.sum(axis=1) + 2.0 ** -40 * mag.sum(axis=1)
        near = np.zeros(ratio.shape, dtype=bool)
        for th in THRESHOLDS:
            near |= (np.abs(ratio / th - 1) < NEAR) & (ratio != th)
    return sums, budget, float(near.mean()) if near.size else 0.0


def _cls(v):
    return "nan" if math.isnan(v) else ("+inf" if v == math.inf else ("-inf" if v == -math.inf else "finite"))


@functools.lru_cache(maxsize=None)
def metrics_case(n_frames, frame_numel, seed):
    """(output, target) [n_frames, frame_numel] on the CPU in [0.1, 5.1), with a band of (0, 0) pixels and three pixels exactly on the thresholds per frame
    where the frame has room; computed once, never modified."""
    g = torch.Generator().manual_seed(1000 * seed + n_frames)
    out, tgt = torch.rand(n_frames, frame_numel, generator=g) * 5 + 0.1, torch.rand(n_frames, frame_numel, generator=g) * 5 + 0.1
    if frame_numel >= 64:
        band = slice(8, 8 + frame_numel // 16)
        out[:, band], tgt[:, band] = 0.0, 0.0
        tgt[:, 1:4] = 1.0
        out[:, 1:4] = torch.tensor(THRESHOLDS, dtype=torch.float32)       # ratio == threshold: not below it
    return out, tgt


def _metrics_call(kind, out, tgt, n_frames=None, scratch=None):
    """fd_depth_metrics (n_frames None) or fd_depth_metrics_frames -> ([rows, 10] fp64 numpy, guard elements touched + inputs changed)"""
    L = harness.get_lib(kind)
    dev = forms.device_of(kind)
    od, td = out.contiguous().to(dev), tgt.contiguous().to(dev)
    rows = n_frames or 1
    sums = Arena(kind, torch.float64, [10 * rows])
    scratch = scratch or _nan_scratch(kind, L.fd_depth_metrics_scratch_bytes() if n_frames is None else L.fd_depth_metrics_frames_scratch_bytes(n_frames))
    if n_frames is None:
        capi.check(L, L.fd_depth_metrics(od.data_ptr(), td.data_ptr(), od.numel(), sums.ptr(), scratch.ptr(), _stream(kind)), "fd_depth_metrics")
    else:
        capi.check(L, L.fd_depth_metrics_frames(od.data_ptr(), td.data_ptr(), n_frames, od.numel() // n_frames, sums.ptr(), scratch.ptr(), _stream(kind)), "fd_depth_metrics_frames")
    bad = sums.bad_guards() + scratch.bad_guards() + int(not (np.array_equal(_bits(od), _bits(out)) and np.array_equal(_bits(td), _bits(tgt))))
    return sums.view().cpu().numpy().reshape(rows, 10).copy(), bad


def _assert_sums(kind, check, case, t0, got, out, tgt, extra=None):
    """One row of ten sums against the fp64 reference: same class everywhere, counts exact, the real-valued sums within their budgets."""
    ref, budget, near = metrics_reference(out.numpy(), tgt.numpy())
    figs = {"near_threshold_share": near}
    for k in range(10):
        if _cls(ref[k]) == "finite" and _cls(got[k]) == "finite":
            figs["dev%d" % k], figs["budget%d" % k] = float(abs(got[k] - ref[k])), float(0.0 if k in COUNT_SUMS else budget[k])
        else:
            figs["class%d" % k] = "%s/%s" % (_cls(got[k]), _cls(ref[k]))
    figs.update(extra or {})
    forms.note(kind, check, case, t0, **figs)
    assert near == 0.0, "pick another seed: pixels within 2^-20 of a threshold"
    for k in range(10):
        assert _cls(got[k]) == _cls(ref[k]), (k, got[k], ref[k])
        if _cls(ref[k]) == "finite":
            assert abs(got[k] - ref[k]) <= (0.0 if k in COUNT_SUMS else budget[k]), (k, got[k], ref[k], budget[k])


def check_metrics_pooled(kind, n_frames, frame_numel, seed):
    t0 = time.time()
    out, tgt = metrics_case(n_frames, frame_numel, seed)
    got, bad = _metrics_call(kind, out, tgt)
    _assert_sums(kind, "metrics_pooled", str(out.numel()), t0, got[0], out, tgt, {"guards_or_inputs_touched": bad})
    assert bad == 0


def check_metrics_frames(kind, n_frames, frame_numel, seed):
    """Every row against its own fp64 reference; rows bit-equal to single-frame calls; totals equal to the pooled call."""
    t0 = time.time()
    out, tgt = metrics_case(n_frames, frame_numel, seed)
    got, bad = _metrics_call(kind, out, tgt, n_frames)
    assert bad == 0
    for f in range(n_frames):
        _assert_sums(kind, "metrics_frames", "%dx%d-frame%d" % (n_frames, frame_numel, f), t0, got[f], out[f], tgt[f])
    for f in range(n_frames):
        one, bad1 = _metrics_call(kind, out[f], tgt[f], 1)
        assert bad1 == 0 and np.array_equal(one[0].view(np.uint64), got[f].view(np.uint64)), "row %d differs from the single-frame call" % f
    pooled, _ = _metrics_call(kind, out, tgt)
    rel = float(np.max(np.abs(got.sum(axis=0) - pooled[0]) / np.maximum(np.abs(pooled[0]), 1e-300)))
    forms.note(kind, "metrics_frames_consistency", "%dx%d" % (n_frames, frame_numel), t0, single_frame_rows_bit_equal=n_frames, totals_vs_pooled_rel=rel, rtol=1e-12)
    assert np.allclose(got.sum(axis=0), pooled[0], rtol=1e-12, atol=0.0)


def check_metrics_scratch_reuse(kind):
    """A short pooled call (2 partial rows) after a long one (1024) on the same scratch: bit for bit the fresh-scratch result."""
    t0 = time.time()
    L = harness.get_lib(kind)
    scratch = _nan_scratch(kind, L.fd_depth_metrics_scratch_bytes())
    _metrics_call(kind, *metrics_case(*METRICS_POOLED[-1]), scratch=scratch)
    short = metrics_case(*METRICS_POOLED[2])
    reused, bad = _metrics_call(kind, *short, scratch=scratch)
    fresh, bad2 = _metrics_call(kind, *short)
    same = np.array_equal(reused.view(np.uint64), fresh.view(np.uint64))
    forms.note(kind, "metrics_scratch_reuse", "262401-then-257", t0, bit_equal=int(same), guards_or_inputs_touched=bad + bad2)
    assert same and bad == 0 and bad2 == 0


@functools.lru_cache(maxsize=None)
def metrics_special_case(name):
    """777 finite pixels (no band, no ties) with five pixels of one special class."""
    g = torch.Generator().manual_seed(77)
    out, tgt = torch.rand(1, 777, generator=g) * 5 + 0.1, torch.rand(1, 777, generator=g) * 5 + 0.1
    at = [0, 63, 64, 500, 776]
    o, t = {"target_zero": ([0.5, 1.0, 2.0, 3.5, 5.0], [0.0] * 5),
            "output_zero": ([0.0] * 5, [0.5, 1.0, 2.0, 3.5, 5.0]),
            "output_negative": ([-0.5, -1.0, -2.0, -3.5, -5.0], [0.5, 1.25, 2.0, 0.1, 5.0]),
            "both_nonpositive": ([0.0, -1.0, -2.0, 0.0, -0.0], [0.0, 0.0, -3.0, -1.0, -0.0]),
            "output_nan": ([float("nan")] * 5, [0.5, 1.0, 2.0, 3.5, 5.0])}[name]
    out[0, at], tgt[0, at] = torch.tensor(o), torch.tensor(t)
    return out, tgt


def check_metrics_special(kind, name):
    t0 = time.time()
    out, tgt = metrics_special_case(name)
    got, bad = _metrics_call(kind, out, tgt)
    _assert_sums(kind, "metrics_special_pooled", name, t0, got[0], out, tgt, {"guards_or_inputs_touched": bad})
    row, bad1 = _metrics_call(kind, out, tgt, 1)
    _assert_sums(kind, "metrics_special_frames", name, t0, row[0], out, tgt, {"guards_or_inputs_touched": bad1})
    assert bad == 0 and bad1 == 0


def check_metrics_all_invalid_frame(kind):
    """3 x 777 with frame 1 all invalid, on a scratch that still holds the partials of a finite batch: the frame's ten sums are exactly 0 and the result's
    fields NaN, for that frame only."""
    import metrics
    t0 = time.time()
    L = harness.get_lib(kind)
    out, tgt = [x.clone() for x in metrics_case(*METRICS_FRAMES[1])]
    scratch = _nan_scratch(kind, L.fd_depth_metrics_frames_scratch_bytes(3))
    _metrics_call(kind, out, tgt, 3, scratch=scratch)
    i = torch.arange(777)
    out[1], tgt[1] = torch.tensor([0.0, -1.0, -0.0])[i % 3], torch.tensor([0.0, -2.0, -0.5, -0.0])[i % 4]
    got, bad = _metrics_call(kind, out, tgt, 3, scratch=scratch)
    assert bad == 0
    for f in (0, 2):
        _assert_sums(kind, "metrics_all_invalid_frame", "frame%d" % f, t0, got[f], out[f], tgt[f])
    zero = bool(np.all(got[1].view(np.uint64) << np.uint64(1) == 0))
    if kind == "hip":
        res = metrics.Result.evaluate_frames(out.to("cuda"), tgt.to("cuda"))
    else:                                                                  # the product's metrics module takes device tensors only: its arithmetic on this tier's sums
        with np.errstate(invalid="ignore", divide="ignore"):
            res = [metrics.Result()._from_sums(s) for s in got]
    fields = [[getattr(r, m) for m in metrics._MEASURES] for r in res]
    nan_rows = [all(math.isnan(v) for v in row) for row in fields]
    any_nan_rows = [any(math.isnan(v) for v in row) for row in fields]
    forms.note(kind, "metrics_all_invalid_frame", "frame1", t0, sums_exactly_zero=int(zero), result_rows_all_nan=str(nan_rows).replace(" ", ""))
    assert zero, got[1]
    assert nan_rows == [False, True, False] and any_nan_rows == [False, True, False]
