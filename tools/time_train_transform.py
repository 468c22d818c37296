"""Times fd_train_transform (the training augmentation) next to fd_val_transform (the validation gather) on the GPU, in one process, with device
events: B = 32 raw 480 x 640 frames -> 224 x 224, depth included.  Alternates the two and reports the median of the rounds, the per-launch times of
the augmentation (fd_trace_*) and the ratio; writes the record to --out (default profiles/train_transform.txt).  Fails without a GPU.

    python tools/time_train_transform.py [--rounds 9] [--iters 200] [--out profiles/train_transform.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-depth_amd"))
from dataloaders import nyu  # noqa: E402
from fastdepth_hip import capi  # noqa: E402
from fastdepth_hip.engine import lib  # noqa: E402

TRAIN_STEP_MS = 2.01         # bf16 train step at B = 32 (README.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_transform.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not estimate")
    n, (H, W), (oh, ow) = a.batch, (nyu.IHEIGHT, nyu.IWIDTH), (224, 224)
    g = torch.Generator(device="cuda").manual_seed(0)
    rgb = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    depth = 0.5 + 9.5 * torch.rand((n, H, W), device="cuda", generator=g)
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    x, d = torch.empty((n, 3, oh, ow), device="cuda"), torch.empty((n, 1, oh, ow), device="cuda")
    ymap, xmap = [torch.from_numpy(t).cuda() for t in nyu.val_index_maps((oh, ow), H, W)]
    rec = nyu.check_train_params(nyu.sample_train_params(n, np.random.RandomState(0)), n)
    p_dev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    scratch = torch.empty(L.fd_train_transform_scratch_bytes(n, oh, ow), dtype=torch.uint8, device="cuda")

    def val():
        capi.check(L, L.fd_val_transform(rgb.data_ptr(), depth.data_ptr(), n, H, W, oh, ow, ymap.data_ptr(), xmap.data_ptr(), x.data_ptr(), d.data_ptr(), stream), "fd_val_transform")

    def train():
        capi.check(L, L.fd_train_transform(rgb.data_ptr(), depth.data_ptr(), n, H, W, oh, ow, p_dev.data_ptr(), x.data_ptr(), d.data_ptr(), scratch.data_ptr(), stream), "fd_train_transform")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in (val, train):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    tv, tt = [], []
    for _ in range(a.rounds):                 # alternate: both see the same neighbours on a shared machine
        tv.append(timed(val))
        tt.append(timed(train))
    # per-launch device times of one augmentation call
    capi.check(L, L.fd_trace_begin(), "fd_trace_begin")
    train()
    recs, cnt = (capi.TraceRecord * 8)(), ctypes.c_int32()
    capi.check(L, L.fd_trace_end(stream, recs, 8, ctypes.byref(cnt)), "fd_trace_end")
    mv, mt = statistics.median(tv), statistics.median(tt)
    lines = ["fd_train_transform vs fd_val_transform, B = %d, %d x %d -> %d x %d, with depth; %s" % (n, H, W, oh, ow, torch.cuda.get_device_name(0)),
             "back-to-back calls between two device events, %d calls per window, median of %d alternating rounds (min .. max)" % (a.iters, a.rounds),
             "fd_val_transform    %.4f ms  (%.4f .. %.4f)" % (mv, min(tv), max(tv)),
             "fd_train_transform  %.4f ms  (%.4f .. %.4f)" % (mt, min(tt), max(tt)),
             "ratio train / val   %.2f" % (mt / mv),
             "share of the bf16 train step (%.2f ms, README.md)  %.1f %%" % (TRAIN_STEP_MS, 100.0 * mt / TRAIN_STEP_MS),
             "one call, per launch (kernel begin/end timestamps):"]
    lines += ["  %-16s %.4f ms" % (recs[i].kernel.decode(), recs[i].ms) for i in range(min(cnt.value, 8))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
