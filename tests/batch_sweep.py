"""The default inference plan at every batch size that changes its kernels: form keys, their enumeration, the committed batch lists and the
device check.  TEST INFRASTRUCTURE ONLY: shared by tests/test_batch_sweep.py (CPU tier: plan creation on the emulator library, no kernel runs)
and tests/test_gpu_batch_sweep.py (kind = "hip": the plans the product selects -- no FD_TUNE_FORCE_* flag, no kept activations -- run on an MI355X).

The plan picks its kernels from M = B * H * W of every map and from how many whole frames fit a workgroup's tile (choose_pw / choose_pw16 /
g16_breg_pick in csrc/fd_plan_select.h, the fusion rules and rows/item in csrc/fd_plan_build.h).  form_key() is a kernel-info line with
the numbers that merely scale with the batch removed, so that two batch sizes share a key exactly when a layer runs the same kernel form.

Regenerate BATCHES, FORM_DIGESTS and the coverage table of DESIGN.md section 4 after moving a threshold:   python tests/batch_sweep.py
(the pruned bf16 drift behind BOUND_REF:   python tests/batch_sweep.py --drift)."""
import functools
import hashlib
import re
import sys
import time

import numpy as np
import torch

import harness
if harness.REPO not in sys.path:          # run as a script: `oracle` is imported from the repository root, as tests/conftest.py arranges for pytest
    sys.path.insert(0, harness.REPO)
import forms  # noqa: E402
from fastdepth_hip import capi
from oracle import inputs, torch_ref

SIZE = 224                      # the thresholds are functions of B * 56^2 ... B * 7^2: a smaller image does not reach the same selections
SWEEP = range(1, 129)           # the batch sizes the CPU tier enumerates
TESTED_BEFORE = (1, 2, 3, 4, 32, 64)      # the batch sizes at which a default 224 x 224 plan ran before this sweep (coverage table)
MAX_LIST = 28
FRAMES, FRAME_SEED = 8, 21

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CONFIGS = [dt + "_" + widths for dt in DTYPES for widths in ("full", "pruned")]

# Greedy set cover of the (layer, form key) pairs of B = 1 ... 128 (cover_batches below), plus 8 and 16 -- the most ordinary sizes a user passes.
BATCHES = {
    "f32_full": [1, 4, 8, 13, 16, 17, 26, 31, 32, 34, 52, 53, 64, 73, 74, 84, 98, 104, 128],
    "f32_pruned": [1, 2, 8, 10, 15, 16, 21, 24, 26, 29, 31, 32, 36, 40, 41, 42, 51, 54, 62, 64, 73, 83, 84, 105, 125, 128],
    "f16_full": [1, 8, 16, 32, 64, 128],
    "f16_pruned": [1, 8, 16, 32, 64, 128],
    "bf16_full": [1, 8, 16, 32, 64, 128],
    "bf16_pruned": [1, 8, 16, 32, 64, 128],
}

# sha1 digest of the sorted (layer, form key) pairs of the default plan at every listed batch size, derived on the emulator library (the CPU
# tier checks them there); the device plan must reproduce them -- the selection is host code with a constant CU count.
FORM_DIGESTS = {
    "f32_full": {1: "6a84c8754d6b", 4: "e863eea83d41", 8: "98f4e5e90047", 13: "7cb47e2119f4", 16: "a1e6ffd7efff", 17: "5daa851b646f",
                 26: "aedf1eb0b564", 31: "9e2f9c686cf6", 32: "83b4d5e9b217", 34: "4b5551693584", 52: "262a71876ccc", 53: "4138146fa18e",
                 64: "7715f4719c80", 73: "23dc835cdc81", 74: "25a37178151d", 84: "441db1000eb3", 98: "a6636eea5566", 104: "f275337e8c8e",
                 128: "922973b3850b"},
    "f32_pruned": {1: "8b623c433d4d", 2: "0ed619ca4970", 8: "68b87c441ea8", 10: "b84164c68344", 15: "519c2749b57f", 16: "519c2749b57f",
                   21: "80b5083f6336", 24: "7d454c584f84", 26: "ffb18aac19f8", 29: "5ff347497900", 31: "c2a6dbf73d94", 32: "b3d25f3d7d73",
                   36: "1db8fb14d710", 40: "97f52d797062", 41: "3aec24faad64", 42: "0e7e42998bdb", 51: "2bfca839e71d", 54: "bdb10a53f099",
                   62: "4488554cb352", 64: "ebc732a02880", 73: "84efcf1dc98e", 83: "d959aa293bd6", 84: "223a75067912", 105: "803196ee6cf5",
                   125: "b222e9365f2c", 128: "ad252e868e83"},
    "f16_full": {1: "e0c893f74a17", 8: "e0c893f74a17", 16: "e0c893f74a17", 32: "e31881b891ca", 64: "512a12d4708a", 128: "e6473a1e5d56"},
    "f16_pruned": {1: "7a8d8415d210", 8: "7a8d8415d210", 16: "7a8d8415d210", 32: "13535e3cbf80", 64: "ec2153824e41", 128: "95457e2be713"},
    "bf16_full": {1: "e0c893f74a17", 8: "e0c893f74a17", 16: "e0c893f74a17", 32: "e31881b891ca", 64: "512a12d4708a", 128: "e6473a1e5d56"},
    "bf16_pruned": {1: "7a8d8415d210", 8: "7a8d8415d210", 16: "7a8d8415d210", 32: "13535e3cbf80", 64: "ec2153824e41", 128: "95457e2be713"},
}

TOL_F32 = forms.TOL             # per frame
ULP = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}     # bound (a): 4 ulp against the first-generation 16-bit kernels (test_16bit_gemm16_fused_epilogues_vs_first_generation_kernels)
# bound (b), 16-bit output against the fp64 reference over the whole batch: the project's bounds (test_16bit_default_plan_batch32_vs_oracle,
# test_pruned_fp16_batch64_config5), which stand at about four times the reference's own 16-bit drift (fp16 9e-4, bf16 7.6e-3).
# bf16_pruned had none: four times BF16_PRUNED_DRIFT, the max-rel error of torch_ref with parameters and activations in bfloat16 on the CPU against
# its fp64 output on the eight frames of this sweep (measure_bf16_drift).
BF16_PRUNED_DRIFT = 6.53e-3
BOUND_REF = {"f16_full": 4e-3, "bf16_full": 3e-2, "f16_pruned": 1e-2, "bf16_pruned": 4 * BF16_PRUNED_DRIFT}


def split(config):
    dt, widths = config.split("_")
    return dt, widths


@functools.lru_cache(maxsize=None)
def module(widths):
    """full: the `base_s0` golden module; pruned: the module of test_pruned_plan_vs_oracle.  Built once, never modified."""
    if widths == "full":
        return inputs.golden_case("base_s0")[0].eval()
    models = inputs.product_models()
    torch.manual_seed(11)
    return harness.randomize_bn(models.MobileNetSkipAdd((SIZE, SIZE), pretrained=False, channels=models.PRUNED_CHANNELS), 12).eval()


# ---- form key ---------------------------------------------------------------------------------------------------------------------------

_GEMM16 = re.compile(r"pw_gemm16<TM=(\d+): (\d+x64 tile), stride (\d+)>")
_DROP = [re.compile(p) for p in (r"\bM=\d+", r"\btiles=\d+x\d+", r"\(\d+\.\d+ per CU\)", r"\bgrid=\d+(x\d+)*", r"\blds=\d+")]
_LAYER = [(re.compile(r"\b(of|into) layer \d+"), r"\1 layer N"), (re.compile(r"\blayer \d+'s"), "layer N's")]


def stride_class(tm, stride):
    return "full" if stride == 16 * tm else ("short/16" if stride < 16 * tm and stride % 16 == 0 else "short/odd")


def form_key(info_line):
    """fd_plan_kernel_info's line without the numbers that scale with the batch: M, the tile counts, the grid, the LDS bytes and the layer
    indices go; a pw_gemm16 stride becomes its class (full tile / short and a multiple of the 16-row MFMA tile / short and odd).  TM, the
    tile, N, K, rows/item, the fused-consumer text and `weight fragments in registers` stay."""
    s = _GEMM16.sub(lambda m: "pw_gemm16<TM=%s: %s, stride %s>" % (m.group(1), m.group(2), stride_class(int(m.group(1)), int(m.group(3)))), info_line)
    for rx in _DROP:
        s = rx.sub("", s)
    for rx, to in _LAYER:
        s = rx.sub(to, s)
    s = re.sub(r"\s+", " ", s)
    s = re.sub(r" ,", ",", s)
    s = re.sub(r"(, ?)+,", ",", s)
    s = re.sub(r", ?\+", " +", s)
    return s.strip(" ,")


# ---- enumeration ------------------------------------------------------------------------------------------------------------------------

def plan_keys(kind, config, b):
    """[(layer name, form key)] of the default plan (no flags, no kept activations) at batch b; plan creation only."""
    dt, widths = split(config)
    x = torch.empty(1, 3, SIZE, SIZE, device=forms.device_of(kind)).expand(b, 3, SIZE, SIZE)     # CPlan reads its shape and device only
    p = harness.CPlan(kind, module(widths), x, keep=False, dtype=DTYPES[dt], pack=False)
    try:
        return [(l.name, form_key(s)) for l, s in zip(p.layers, p.info())]
    finally:
        p.close()


def enumerate_forms(kind, config, batches):
    """{(layer, form key): set of the batch sizes whose default plan runs that layer in that form}"""
    out = {}
    for b in batches:
        for pair in plan_keys(kind, config, b):
            out.setdefault(pair, set()).add(b)
    return out


def digest(pairs):
    return hashlib.sha1("\n".join(sorted("%s|%s" % p for p in pairs)).encode()).hexdigest()[:12]


def cover_batches(table, always=(8, 16)):
    """Greedy set cover: the batch size that hits the most (layer, key) pairs not hit yet, the smallest on a tie, until all are hit."""
    left, chosen = set(table), []
    while left:
        gain = {}
        for pair in left:
            for b in table[pair]:
                gain[b] = gain.get(b, 0) + 1
        b = min(gain, key=lambda q: (-gain[q], q))
        chosen.append(b)
        left = {pair for pair in left if b not in table[pair]}
    return sorted(set(chosen) | set(always))


def uncovered(table, batches):
    """[(layer, key, a batch size that reaches it)] of the pairs no listed batch size hits"""
    have = set(batches)
    return sorted((layer, key, min(bs)) for (layer, key), bs in table.items() if not (bs & have))


def coverage_row(table):
    """(distinct plans, (layer, form) pairs, pairs at the batch sizes tested before this sweep)"""
    per_b = {}
    for pair, bs in table.items():
        for b in bs:
            per_b.setdefault(b, set()).add(pair)
    return len({frozenset(v) for v in per_b.values()}), len(table), sum(1 for bs in table.values() if bs & set(TESTED_BEFORE))


# ---- reference and inputs ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference(widths):
    """(eight distinct frames, their fp64 torch_ref outputs): computed once per module, shared by every case, never modified.  Eval-mode
    frames are independent, so the reference of a batch is the reference of its frames."""
    frames = inputs.batch_variants(inputs.load_sample()[0], FRAMES, FRAME_SEED)
    p64 = torch_ref.params_from_state(module(widths).state_dict(), dtype=torch.float64)
    with torch.no_grad():
        ref = torch_ref.forward(p64, frames.double())
    return frames, ref.numpy()


def frame_of(n):
    """Slot n of a batch holds frame (5 n + 3) % 8: neighbouring slots differ, and a frame that lands in the wrong slot cannot match its reference."""
    return (5 * n + 3) % FRAMES


def measure_bf16_drift(widths="pruned"):
    """The reference's own bf16 drift on this sweep's frames: torch_ref with parameters and activations in bfloat16 on the CPU against fp64."""
    frames, ref = reference(widths)
    p16 = torch_ref.params_from_state(module(widths).state_dict(), dtype=torch.bfloat16)
    with torch.no_grad():
        y = torch_ref.forward(p16, frames.bfloat16()).float().numpy()
    return harness.rel_err(y, ref)


# ---- the device check -------------------------------------------------------------------------------------------------------------------

def _frame_errs(y, ref_b):
    return [harness.rel_err(y[n], ref_b[n]) for n in range(len(ref_b))]


def check_batch(kind, config, b):
    """One (configuration, batch size) case: the default plan's form keys, run-to-run bit equality, and the output against the fp64 reference
    (fp32: every frame on its own; 16 bit: against the first-generation kernels of the same storage type and against fp64)."""
    t0 = time.time()
    dt, widths = split(config)
    dtype, dev = DTYPES[dt], forms.device_of(kind)
    frames, ref = reference(widths)
    idx = [frame_of(n) for n in range(b)]
    x = frames[idx].to(dev)
    ref_b = ref[idx]
    m = module(widths)

    def run(flags):
        p = harness.CPlan(kind, m, x, keep=False, dtype=dtype, flags=flags)
        try:
            return p.info(), [(l.name, form_key(s)) for l, s in zip(p.layers, p.info())], p.forward(x).cpu().numpy(), p.forward(x).cpu().numpy()
        finally:
            p.close()

    info, keys, y, y2 = run(0)
    want = enumerate_forms(kind, config, [b])
    assert set(keys) == set(want), "B=%d: the plan that ran and the enumeration disagree: %s" % (b, sorted(set(keys) ^ set(want)))
    assert digest(keys) == FORM_DIGESTS[config][b], "B=%d: the device plan's forms are not the ones the CPU tier derived (digest %s, committed %s):\n%s" % (
        b, digest(keys), FORM_DIGESTS[config][b], "\n".join(info))
    errs = _frame_errs(y, ref_b)
    worst = int(np.argmax(errs))
    figures = {"frame_worst": errs[worst]}
    checks = {}           # name -> (figure of an output, bound)
    if dt == "f32":
        checks["per-frame rel_err vs fp64"] = (lambda out, _: max(_frame_errs(out, ref_b)), TOL_F32)
    else:
        _, _, y_old, _ = run(capi.FD_PLAN_NO_GEMM16 | capi.FD_PLAN_NO_EPILOGUE_FUSION)
        checks["rel_err vs the first-generation 16-bit kernels"] = (lambda out, old: harness.rel_err(out, old), 4 * ULP[dt])
        checks["batch rel_err vs fp64"] = (lambda out, _: harness.rel_err(out, ref_b), BOUND_REF[config])
        figures["ab"] = harness.rel_err(y, y_old)
        figures["batch"] = harness.rel_err(y, ref_b)
    forms.note(kind, "batch_sweep", "%s-B%d" % (config, b), t0, forms=len({k for _, k in keys}), **figures)
    assert np.array_equal(y, y2), "B=%d: the forward is not reproducible run to run (%d elements differ)" % (b, int((y != y2).sum()))
    for name, (fig, bound) in checks.items():
        got = fig(y, y_old if dt != "f32" else None)
        if got < bound:
            continue
        # which switch removes the failure: each tried once on the same input, so that the failing form can be read off this message
        tried = []
        for fname in ("FD_PLAN_NO_GEMM16", "FD_PLAN_NO_EPILOGUE_FUSION", "FD_PLAN_NO_UNIT_FUSION"):
            try:
                e = fig(run(getattr(capi, fname))[2], y_old if dt != "f32" else None)
                tried.append("%s: %s (%.3g)" % (fname, "passes" if e < bound else "fails", e))
            except Exception as ex:                    # noqa: BLE001  (the message below must still be raised)
                tried.append("%s: %r" % (fname, ex))
        raise AssertionError("%s B=%d: %s = %.3g, bound %.3g; worst frame: slot %d (frame %d) at %.3g vs fp64\n%s\nplan:\n%s" % (
            config, b, name, got, bound, worst, idx[worst], errs[worst], "\n".join(tried), "\n".join("%2d %s" % (i, s) for i, s in enumerate(info))))
    return figures


# ---- regeneration -----------------------------------------------------------------------------------------------------------------------

def _fmt(name, d, per_line=8):
    out = ["%s = {" % name]
    for k, v in d.items():
        if isinstance(v, dict):
            items = ["%d: \"%s\"" % kv for kv in v.items()]
            out.append("    \"%s\": {%s}," % (k, (",\n" + " " * (len(k) + 9)).join(", ".join(items[i:i + per_line]) for i in range(0, len(items), per_line))))
        else:
            out.append("    \"%s\": %s," % (k, v))
    return "\n".join(out + ["}"])


def main(argv):
    if "--drift" in argv:
        d = measure_bf16_drift()
        print("BF16_PRUNED_DRIFT = %.3g    (bound: 4 x = %.3g)" % (d, 4 * d))
        return
    lists, digests = {}, {}
    print("| configuration | distinct plans | (layer, kernel form) pairs | pairs at B in {%s} | batch sizes run |" % ",".join(map(str, TESTED_BEFORE)))
    print("|---|---|---|---|---|")
    for config in CONFIGS:
        per_b = {b: plan_keys("emu", config, b) for b in SWEEP}
        table = {}
        for b, pairs in per_b.items():
            for pair in pairs:
                table.setdefault(pair, set()).add(b)
        lists[config] = cover_batches(table)
        digests[config] = {b: digest(per_b[b]) for b in lists[config]}
        print("| %s | %d | %d | %d | %d |" % ((config,) + coverage_row(table) + (len(lists[config]),)))
    print(_fmt("BATCHES", lists))
    print(_fmt("FORM_DIGESTS", digests, per_line=6))


if __name__ == "__main__":
    main(sys.argv[1:])
