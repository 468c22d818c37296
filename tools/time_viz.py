"""Times fd_depth_rows (the comparison rows `rgb | target | prediction` painted on the device) at B = 32, 224 x 224, k = 2, in one process with device
events: the call, its two launches (fd_trace_*), the host route it replaces (three .cpu().numpy() copies + the NumPy restatement tests/viz_ref.py, which
is cheaper than the reference's matplotlib route) and the fp32 forward for scale.  Writes the record to --out (default profiles/viz_rows.txt).
Fails without a GPU.

    python tools/time_viz.py [--rounds 9] [--iters 200] [--out profiles/viz_rows.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-depth_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import models  # noqa: E402
import viz_ref  # noqa: E402
from fastdepth_hip import capi, viz  # noqa: E402
from fastdepth_hip.engine import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "viz_rows.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not estimate")
    n, h, w = a.batch, 224, 224
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((n, 3, h, w), device="cuda", generator=g)
    target = 0.7 + 9.3 * torch.rand((n, 1, h, w), device="cuda", generator=g)
    torch.manual_seed(0)
    model = models.MobileNetSkipAdd((h, w), pretrained=False)
    model.decode_conv6[1].bias.data.fill_(2.8)
    model = model.cuda().eval()
    with torch.no_grad():
        pred = model(x)
    canvas = torch.empty((n * h, 3 * w, 3), dtype=torch.uint8, device="cuda")
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream

    def rows():
        viz.paint_rows(x, target, pred, out=canvas)

    def forward():
        with torch.no_grad():
            model(x)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in (rows, forward):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    tr, tf = [], []
    for _ in range(a.rounds):                 # alternate: both see the same neighbours on a shared machine
        tr.append(timed(rows))
        tf.append(timed(forward))
    capi.check(L, L.fd_trace_begin(), "fd_trace_begin")
    rows()
    recs, cnt = (capi.TraceRecord * 8)(), ctypes.c_int32()
    capi.check(L, L.fd_trace_end(stream, recs, 8, ctypes.byref(cnt)), "fd_trace_end")
    # the host route: wall-clock, synchronised, three times
    th = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xa, ta, pa = x.cpu().numpy(), target.cpu().numpy(), pred.cpu().numpy()
        ref = viz_ref.paint_rows(xa, [ta, pa])
        th.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    same = bool((canvas.cpu().numpy() == ref).all())
    mr, mf = statistics.median(tr), statistics.median(tf)
    lines = ["fd_depth_rows, B = %d, %d x %d, rgb | target | prediction (k = 2); %s" % (n, h, w, torch.cuda.get_device_name(0)),
             "back-to-back calls between two device events, %d calls per window, median of %d alternating rounds (min .. max)" % (a.iters, a.rounds),
             "viz.paint_rows (fd_depth_rows)   %.4f ms  (%.4f .. %.4f)   = %.2f us per frame" % (mr, min(tr), max(tr), 1e3 * mr / n),
             "fp32 forward                     %.4f ms  (%.4f .. %.4f)" % (mf, min(tf), max(tf)),
             "rows / forward                   %.3f" % (mr / mf),
             "one call, per launch (kernel begin/end timestamps):"]
    lines += ["  %-16s %.4f ms" % (recs[i].kernel.decode(), recs[i].ms) for i in range(min(cnt.value, 8))]
    lines += ["host route (3 x .cpu().numpy() + NumPy restatement), wall clock, best of 3:  %.1f ms  = %.2f ms per frame" % (min(th), min(th) / n),
              "device canvas == host route: %s" % same]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
