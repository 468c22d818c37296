"""Times the bilinear launches (fd_dwb_rows, FD_OP_DWB; fd_head_bilinear, FD_OP_PWB) of MobileNet('blconv5dw' / 'blconv3dw') at B = 32,
224 x 224, in fp32 and fp16, in one process: every launch under fd_trace_* (kernel begin/end timestamps) with its algorithmic bytes
(fd_plan_layer_stats), bytes/s and share of the HBM peak; in the same run, as the yardstick, the transposed depthwise launches (fd_dwt_rows) of
MobileNet('deconv5dw' / 'deconv3dw'), which also read a map once and write the four times larger one (decoder.convtJ.0 writes the map of
decoder.convJ.0 with twice the channels, so compare bytes/s, or the time of convtJ.0 with that of conv(J+1).0); and whole-forward frames/s of the
models beside MobileNet('nnconv5dw').  Writes the record to --out (default profiles/bilinear_rows.txt).  Recorded, not asserted.  Fails without a GPU.

    python tools/time_bilinear.py [--batch 32] [--traces 5] [--iters 50] [--out profiles/bilinear_rows.txt]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-depth_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import models  # noqa: E402
from time_shuffle import HBM_PEAK, frames_per_s, traced  # noqa: E402

KERNELS = ("fd_dwb_rows", "fd_head_bilinear", "fd_dwt_rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--traces", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bilinear_rows.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not estimate")
    x = torch.rand((a.batch, 3, 224, 224), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    lines = ["bilinear launches, B = %d, 224 x 224; %s" % (a.batch, torch.cuda.get_device_name(0)),
             "per launch: kernel begin/end timestamps under fd_trace_*, median of %d traced forwards; bytes = fd_plan_layer_stats (one read of the producer's map, one "
             "write of the output, weights, bias); share of the %.1f TB/s HBM specification" % (a.traces, HBM_PEAK / 1e12),
             "frames/s: %d back-to-back forwards between two device events" % a.iters]
    for dtype in (torch.float32, torch.float16):
        for name in ("blconv5dw", "blconv3dw", "deconv5dw", "deconv3dw", "nnconv5dw"):
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
                if not sym.startswith(KERNELS):
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
