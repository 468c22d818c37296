"""Comparison rows on a real MI355X: viz.paint_rows == the NumPy restatement (tests/viz_ref.py: no matplotlib, no PIL, no reference tree) byte for
byte on the shared cases and on the golden sample -- which is what a division that is not IEEE, a minimum that drops a NaN, contraction, or a wrong
combination of the workgroups' partial ranges would break -- and evaluate.validate with the comparison option end to end."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import viz_ref

pytestmark = pytest.mark.gpu

PREFILL = 0xA5


def paint(c):
    from fastdepth_hip import viz
    x = torch.from_numpy(np.array(c["x"], np.float32)).cuda() if c["x"] is not None else None
    maps = [torch.from_numpy(np.array(m, np.float32)).cuda() for m in c["maps"]]
    n, h, w = maps[0].shape[0], maps[0].shape[-2], maps[0].shape[-1]
    row = (len(maps) + (x is not None)) * w * 3
    pitch = row + c["pitch_extra"]
    buf = torch.full((n * h, pitch), PREFILL, dtype=torch.uint8, device="cuda")
    # a view of the padded canvas: rows `pitch` bytes apart, pixels contiguous
    out = torch.as_strided(buf, (n * h, row // 3, 3), (pitch, 3, 1))
    got = viz.paint_rows(x, *maps, value_range=c["value_range"], out=out)
    assert got.data_ptr() == buf.data_ptr()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), row


@pytest.mark.parametrize("name", ("A", "B", "C", "D", "E", "F"))
def test_gpu_depth_rows_equal_the_restatement(name):
    c = viz_ref.cases()[name]
    canvas, row = paint(c)
    want = viz_ref.want(name)
    got = canvas[:, :row].reshape(want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    assert (canvas[:, row:] == PREFILL).all(), name                 # bytes beyond the panels keep their prefill
    again, _ = paint(c)
    assert again.tobytes() == canvas.tobytes(), name


def test_gpu_nan_frame_leaves_its_neighbours_alone():
    d, _ = paint(viz_ref.cases()["D"])
    clean, _ = paint(viz_ref.cases()["D_clean"])
    assert np.array_equal(d[:8], clean[:8]) and np.array_equal(d[16:], clean[16:])
    assert np.array_equal(d[8:16, :36], clean[8:16, :36]) and not d[8:16, 36:].any() and clean[8:16, 36:].any()


def test_gpu_golden_sample_and_fresh_canvas():
    from fastdepth_hip import viz
    x, d, p = [torch.from_numpy(a).cuda() for a in viz_ref.sample()]
    out = viz.paint_rows(x, d, p)
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == (224, 672, 3)
    assert np.array_equal(out.cpu().numpy(), np.load(os.path.join(viz_ref.GOLD, "viz_sample_row.npy")))
    one = viz.paint_rows(None, d[0, 0])                             # colored_depthmap: one [h, w] map, no colour panel
    lo, hi = viz_ref.frame_range([d[0, 0].cpu().numpy()])
    assert np.array_equal(one.cpu().numpy(), viz_ref.colour(d[0, 0].cpu().numpy(), lo, hi))


def test_gpu_utils_drop_in(tmp_path):
    import utils
    x, d, p = viz_ref.sample()
    gold = np.load(os.path.join(viz_ref.GOLD, "viz_sample_row.npy"))
    row = utils.merge_into_row(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(p).cuda())
    assert isinstance(row, np.ndarray) and row.dtype == np.uint8 and np.array_equal(row, gold)
    assert np.array_equal(utils.merge_into_row(x, d, p), gold)      # NumPy inputs are uploaded
    img = utils.add_row(row, row)
    utils.save_image(img, str(tmp_path / "c.png"))
    assert np.array_equal(viz_ref.png_decode(open(str(tmp_path / "c.png"), "rb").read()), img)


_TIMES = re.compile(r"t_GPU=[0-9.]+(\([0-9.]+\))?")


@pytest.mark.parametrize("batch", (2, 3))
def test_gpu_evaluate_comparison_image(tmp_path, capsys, batch):
    """evaluate.validate on 5 synthetic 64 x 64 frames, skip 2: frames 0, 2, 4 -- with batch size 2 in three different batches, with batch size 3 at the
    in-batch positions 0, 2, 1.  The written PNG, decoded, equals viz_ref on the same inputs and on model(inp) recomputed here; the metrics returned
    and the printout equal those of a run without the option (t_GPU is wall-clock time and differs between any two runs: it is masked in the text
    and left out of the compared fields)."""
    import evaluate
    import models
    torch.manual_seed(11)
    model = models.MobileNetSkipAdd((64, 64), pretrained=False)
    model.decode_conv6[1].bias.data.fill_(2.8)
    model = model.cuda().eval()
    g = np.random.default_rng(5)
    samples = [(torch.from_numpy(g.random((3, 64, 64), dtype=np.float32)), torch.from_numpy((0.7 + 9.3 * g.random((1, 64, 64), dtype=np.float32)).astype(np.float32)))
               for _ in range(5)]
    device = torch.device("cuda", 0)
    path = str(tmp_path / "comparison.png")

    def run(**kw):
        args = argparse.Namespace(batch_size=batch, print_freq=1, **kw)
        avg = evaluate.validate(samples, model, args, device)
        return avg, _TIMES.sub("t_GPU=*", capsys.readouterr().out)

    plain, plain_out = run()
    assert not os.path.exists(path)
    with_img, img_out = run(comparison=path, comparison_skip=2)
    assert img_out == plain_out and "RMSE=" in plain_out
    for k in ("rmse", "mae", "delta1", "delta2", "delta3", "absrel", "lg10", "irmse", "imae", "mse"):
        assert getattr(with_img, k) == getattr(plain, k), k
    img = viz_ref.png_decode(open(path, "rb").read())
    assert img.shape == (3 * 64, 3 * 64, 3) and np.array_equal(img, evaluate.validate.img_merge) and evaluate.validate.img_merge.dtype == np.uint8
    rows = []
    for f in (0, 2, 4):
        b0 = f // batch * batch                                     # the batch the frame fell in, evaluated as the loop evaluated it
        inp = torch.stack([s[0] for s in samples[b0:b0 + batch]]).cuda()
        with torch.no_grad():
            pred = model(inp)
        rows.append(viz_ref.paint_rows(samples[f][0][None].numpy(), [samples[f][1][None].numpy(), pred[f - b0:f - b0 + 1].cpu().numpy()]))
    assert np.array_equal(img, np.vstack(rows))
