"""Times the dense convolution launches (fd_conv_gemm + fd_conv_reduce, FD_OP_CONV) of MobileNet('nnconv5' / 'nnconv3') at B = 32, 224 x 224, in fp32
and fp16, in one process: every conv layer under fd_trace_* (kernel begin/end timestamps; a split-K layer's two launches are added) with its
algorithmic FLOPs and bytes (fd_plan_layer_stats), TFLOP/s and share of the dtype's MFMA peak; in the same run the pointwise launches of
MobileNetSkipAdd on fd_pw_gemm_f32 / fd_pw_gemm_h16 as a yardstick; whole-forward frames/s; and the two error ratios of the layer-local test
(tests/dense_ref.py) for decoder.conv1 of nnconv5 on a 3 x 5 map.  Writes the record to --out (default profiles/dense_conv.txt).  Recorded, not
asserted.  Fails without a GPU.

    python tools/time_dense.py [--batch 32] [--traces 5] [--iters 20] [--out profiles/dense_conv.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-depth_amd"))
import models  # noqa: E402
from fastdepth_hip import capi  # noqa: E402
from fastdepth_hip.engine import lib  # noqa: E402

MFMA_PEAK = {torch.float32: 157.3e12, torch.float16: 2500.0e12}      # FLOP/s: the dense fp32 and fp16 MFMA peaks bench.py prices against


def traced(model, x, rounds):
    """{layer index: (kernel names in launch order, median over `rounds` traced forwards of the summed ms of the layer's launches)}"""
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    seen = {}
    for _ in range(rounds):
        capi.check(L, L.fd_trace_begin(), "fd_trace_begin")
        with torch.no_grad():
            model(x)
        recs, cnt = (capi.TraceRecord * 256)(), ctypes.c_int32()
        capi.check(L, L.fd_trace_end(stream, recs, 256, ctypes.byref(cnt)), "fd_trace_end")
        one = {}
        for i in range(min(cnt.value, 256)):
            names, ms = one.setdefault(recs[i].layer, ([], 0.0))
            one[recs[i].layer] = (names + [recs[i].kernel.decode()], ms + recs[i].ms)
        for k, (names, ms) in one.items():
            seen.setdefault(k, (names, []))[1].append(ms)
    return {k: (v[0], statistics.median(v[1])) for k, v in seen.items()}


def frames_per_s(model, x, iters):
    with torch.no_grad():
        for _ in range(3):
            model(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            model(x)
        e1.record()
        e1.synchronize()
    return x.shape[0] * iters / (e0.elapsed_time(e1) * 1e-3)


def rho_lines():
    """The layer-local ratios of tests/dense_ref.py for decoder.conv1 (1024 -> 512, k 5) on a 3 x 5 map, fp32 plan."""
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import dense_ref
    plan, _ = dense_ref.executed("gpu", "nnconv5", dense_ref.SHAPES[1], torch.float32)
    worst, n_over, st, rho, rho_ref = dense_ref.plan_conv_excess(plan, 27)
    return ["", "layer-local error of decoder.conv1 (1024 -> 512, k 5, 3 x 5 map, n = 25 600), fp32 plan, in units of 2^-24 A (tests/dense_ref.py):",
            "  rho_engine = %.3g   rho_ref (torch conv2d, fp32) = %.3g   limit 16 max(rho_ref, 1) = %.3g   worst |y - r| / hard bound = %.3g"
            % (rho, rho_ref, 16 * max(rho_ref, 1.0), worst)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--traces", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dense_conv.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not estimate")
    x = torch.rand((a.batch, 3, 224, 224), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    lines = ["dense convolution launches (implicit GEMM, FD_OP_CONV), B = %d, 224 x 224" % a.batch,
             "per layer: kernel begin/end timestamps under fd_trace_*, median of %d traced forwards (a split-K layer: fd_conv_gemm + fd_conv_reduce added); "
             "GFLOP and MB = fd_plan_layer_stats (2 k^2 cin cout per output pixel; one read of the stored input, one write of the output, weights, bias); "
             "share of the MFMA peak: %.1f TFLOP/s fp32, %.1f TFLOP/s fp16" % (a.traces, MFMA_PEAK[torch.float32] / 1e12, MFMA_PEAK[torch.float16] / 1e12),
             "frames/s: %d back-to-back forwards between two device events" % a.iters]
    for dtype in (torch.float32, torch.float16):
        rates = {}
        for name in ("nnconv5", "nnconv3", "skipadd"):
            torch.manual_seed(0)
            m = models.MobileNetSkipAdd((224, 224), pretrained=False) if name == "skipadd" else models.MobileNet(name, (224, 224), pretrained=False)
            m = m.cuda().eval()
            m.set_compute_dtype(dtype)
            with torch.no_grad():
                m(x)
            stats = m._engine().layer_stats(x)
            tr = traced(m, x, a.traces)
            fps = frames_per_s(m, x, a.iters)
            lines.append("")
            lines.append("%s, %s: %.0f frames/s" % ("MobileNetSkipAdd" if name == "skipadd" else "MobileNet('%s')" % name, str(dtype).replace("torch.", ""), fps))
            tot_f = tot_ms = 0.0
            for i, (lname, sym, info, nbytes, flops) in enumerate(stats):
                # the yardstick: the pointwise launches of MobileNetSkipAdd on the first-generation GEMMs fd_pw_gemm_f32 / fd_pw_gemm_h16
                want = sym.startswith(("fd_pw_gemm_f32<", "fd_pw_gemm_h16<")) if name == "skipadd" else sym.startswith("fd_conv_gemm<")
                if not want or i not in tr:
                    continue
                kern, ms = tr[i]
                tot_f += flops
                tot_ms += ms
                rate = flops / (ms * 1e-3)
                lines.append("  %-18s %-40s %8.4f ms  %8.3f GFLOP  %7.2f TFLOP/s  %5.1f %% of peak  %8.2f MB%s" %
                             (lname, sym, ms, flops / 1e9, rate / 1e12, 100.0 * rate / MFMA_PEAK[dtype], nbytes / 1e6,
                              "  (%d launches)" % len(kern) if len(kern) > 1 else ""))
            rates[name] = tot_f / (tot_ms * 1e-3) if tot_ms else 0.0
            lines.append("  sum: %.3f GFLOP in %.4f ms = %.2f TFLOP/s" % (tot_f / 1e9, tot_ms, rates[name] / 1e12))
            del m
        for name in ("nnconv5", "nnconv3"):
            lines.append("%s, %s: the five convolutions reach %.2f x the pointwise yardstick of the same run (expectation: >= 0.5)" %
                         (name, str(dtype).replace("torch.", ""), rates[name] / rates["skipadd"] if rates["skipadd"] else float("nan")))
    lines += rho_lines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
