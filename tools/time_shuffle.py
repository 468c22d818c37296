"""Times the pixel-shuffle launches (fd_dws_rows, FD_OP_DWS; fd_head_shuffle, FD_OP_PWS) of MobileNet('shuffle5dw' / 'shuffle3dw') at B = 32,
224 x 224, in fp32 and fp16, in one process: every launch under fd_trace_* (kernel begin/end timestamps) with its algorithmic bytes
(fd_plan_layer_stats), bytes/s and share of the HBM peak; in the same run, for scale, the 5x5 depthwise launches of MobileNet('nnconv5dw') on the same
maps (decoder.conv2.0 .. conv5.0: 14 x 14 .. 112 x 112); and whole-forward frames/s of the models.  Writes the record to --out (default
profiles/shuffle_rows.txt).  Recorded, not asserted.  Fails without a GPU.

    python tools/time_shuffle.py [--batch 32] [--traces 5] [--iters 50] [--out profiles/shuffle_rows.txt]
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

HBM_PEAK = 8.0e12          # bytes/s, HBM3E specification of the MI355X (6.3e12 is what a float4 copy achieves)


def traced(model, x, rounds):
    """{layer index: (kernel name, median ms over `rounds` traced forwards)}"""
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    seen = {}
    for _ in range(rounds):
        capi.check(L, L.fd_trace_begin(), "fd_trace_begin")
        with torch.no_grad():
            model(x)
        recs, cnt = (capi.TraceRecord * 128)(), ctypes.c_int32()
        capi.check(L, L.fd_trace_end(stream, recs, 128, ctypes.byref(cnt)), "fd_trace_end")
        for i in range(min(cnt.value, 128)):
            seen.setdefault(recs[i].layer, (recs[i].kernel.decode(), []))[1].append(recs[i].ms)
    return {k: (v[0], statistics.median(v[1])) for k, v in seen.items()}


def frames_per_s(model, x, iters):
    with torch.no_grad():
        for _ in range(10):
            model(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            model(x)
        e1.record()
        e1.synchronize()
    return x.shape[0] * iters / (e0.elapsed_time(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--traces", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shuffle_rows.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not estimate")
    x = torch.rand((a.batch, 3, 224, 224), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    lines = ["pixel-shuffle launches, B = %d, 224 x 224; %s" % (a.batch, torch.cuda.get_device_name(0)),
             "per launch: kernel begin/end timestamps under fd_trace_*, median of %d traced forwards; bytes = fd_plan_layer_stats (one read of the producer's map, one "
             "write of the output, weights, bias); share of the %.1f TB/s HBM specification" % (a.traces, HBM_PEAK / 1e12),
             "frames/s: %d back-to-back forwards between two device events" % a.iters]
    for dtype in (torch.float32, torch.float16):
        for name in ("shuffle5dw", "shuffle3dw", "nnconv5dw"):
            torch.manual_seed(0)
            m = models.MobileNet(name, (224, 224), pretrained=False).cuda().eval()
            m.set_compute_dtype(dtype)
            with torch.no_grad():
                m(x)
            stats = m._engine().layer_stats(x)
            tr = traced(m, x, a.traces)
            fps = frames_per_s(m, x, a.iters)
            lines.append("")
            lines.append("MobileNet('%s'), %s: %.0f frames/s" % (name, str(dtype).replace("torch.", ""), fps))
            for i, (lname, sym, info, nbytes, flops) in enumerate(stats):
                # for scale: the 5x5 depthwise layers of the NNConv sibling on the same maps (they read a quarter of the pixels through nearest x2)
                if not (lname in ["decoder.conv%d.0" % j for j in range(2, 6)] if name == "nnconv5dw" else sym.startswith(("fd_dws_rows", "fd_head_shuffle"))):
                    continue
                if i not in tr:
                    lines.append("  %-18s (no launch of its own: %s)" % (lname, info))
                    continue
                kern, ms = tr[i]
                lines.append("  %-18s %-34s %8.4f ms  %9.3f MB  %6.3f TB/s  %5.1f %% of HBM peak" %
                             (lname, sym, ms, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12, 100.0 * nbytes / (ms * 1e-3) / HBM_PEAK))
            del m
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
