"""Comparison rows (reference utils.py:37-83, deploy/data/visualize.py:22-31) on the CPU tier: the table fixture, the NumPy restatement
tests/viz_ref.py against the golden row and against the reference itself, fd_depth_rows -- its kernels compiled for the emulator -- against the
restatement byte for byte, the error paths, the drop-in utils module, the PNG writer and evaluate's frame selection."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import harness
import viz_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("A", "B", "C", "D", "E", "F")
PREFILL = 0xA5


def run_emu(x, maps, value_range=None, pitch_extra=0, scratch=None, misalign=0):
    """fd_depth_rows of the emulator build on NumPy inputs -> the whole canvas [n * h, pitch] uint8 (prefilled with PREFILL).
    misalign: byte offset of the canvas inside its buffer (an odd one forces the byte path even where the sizes allow dword stores)."""
    L = harness.get_lib("emu")
    maps = [torch.from_numpy(np.array(m, np.float32)) for m in maps]
    n, h, w = maps[0].shape[0], maps[0].shape[-2], maps[0].shape[-1]
    xt = torch.from_numpy(np.array(x, np.float32)) if x is not None else None
    rt = torch.from_numpy(np.array(value_range, np.float32)) if value_range is not None else None
    panels = len(maps) + (1 if x is not None else 0)
    pitch = panels * w * 3 + pitch_extra
    buf = torch.full((n * h * pitch + 64,), PREFILL, dtype=torch.uint8)
    off = (-buf.data_ptr()) % 16 + misalign
    if scratch is None:
        scratch = torch.empty(max(1, L.fd_depth_rows_scratch_bytes(n)), dtype=torch.uint8)
    ptr = [m.data_ptr() for m in maps] + [None] * (3 - len(maps))
    rc = L.fd_depth_rows(xt.data_ptr() if xt is not None else None, ptr[0], ptr[1], ptr[2], n, h, w, rt.data_ptr() if rt is not None else None,
                         buf.data_ptr() + off, pitch, scratch.data_ptr(), None)
    assert rc == 0, L.fd_last_error().decode()
    before, after = buf[:off].numpy(), buf[off + n * h * pitch:].numpy()
    assert (before == PREFILL).all() and (after == PREFILL).all()
    return buf[off:off + n * h * pitch].numpy().reshape(n * h, pitch).copy()


def check_canvas(canvas, want, name):
    row = want.shape[1] * 3
    got = canvas[:, :row].reshape(want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    assert (canvas[:, row:] == PREFILL).all(), name           # bytes beyond the panels keep their prefill


def test_table_fixture_is_matplotlibs_viridis():
    plt = pytest.importorskip("matplotlib.pyplot", reason="matplotlib is not installed (the fixture was generated from it)")
    assert np.array_equal(viz_ref.table(), (255 * plt.cm.viridis(np.arange(256))[:, :3]).astype("uint8"))


def test_embedded_table_equals_the_fixture():
    """A 1 x 256 ramp 0, 1, ..., 255 with range (0, 255 * 256 / 255 = 256): rel * 256 = i exactly, every entry once."""
    ramp = np.arange(256, dtype=np.float32).reshape(1, 1, 1, 256)
    rng = np.array([[0.0, 256.0]], np.float32)
    t = ((ramp - rng[0, 0]) / (rng[0, 1] - rng[0, 0]) * np.float32(256.0)).reshape(-1)
    assert np.array_equal(t, np.arange(256, dtype=np.float32))
    got = run_emu(None, [ramp], rng).reshape(256, 3)
    assert np.array_equal(got, viz_ref.table())


def test_restatement_equals_the_golden_sample_row():
    gold = np.load(os.path.join(viz_ref.GOLD, "viz_sample_row.npy"))
    assert gold.shape == (224, 672, 3) and gold.dtype == np.uint8
    assert np.array_equal(viz_ref.want("sample"), gold)


def test_restatement_equals_the_reference_itself():
    """Cases A-E through the reference's own utils.py (when its tree and matplotlib are present), NumPy warnings silenced.  One stated exception, in
    tools/make_golden_viz.py:compare_with_reference: the reference joins the maps' ranges with Python's min / max, which drop a NaN that is not in the
    first map, while this project propagates it from any map (case D: 573 bytes of frame 1's depth panels differ for that reason alone); the same frame
    with the maps in the other order is compared in full."""
    pytest.importorskip("matplotlib")
    root = os.environ.get("FD_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(root, "utils.py")):
        pytest.skip("reference tree not present")
    spec = importlib.util.spec_from_file_location("make_golden_viz", os.path.join(REPO, "tools", "make_golden_viz.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.compare_with_reference(tool.reference_utils(), viz_ref)


def test_cases_cover_what_they_are_meant_to():
    c = viz_ref.cases()
    assert not viz_ref.want("C").any()                                        # a constant frame is black
    d, clean = viz_ref.want("D"), viz_ref.want("D_clean")
    assert not d[8:16, 12:].any() and np.array_equal(d[8:16, :12], clean[8:16, :12]) and clean[8:16, 12:].any()
    assert np.array_equal(d[:8], clean[:8]) and np.array_equal(d[16:], clean[16:])
    e = viz_ref.want("E")
    tab = viz_ref.table()
    for f in range(2):
        assert tuple(e[f * 8, 12 + 0]) == tuple(tab[255]) and tuple(e[f * 8, 24 + 1]) == tuple(tab[0])       # d == d_max -> 255, d == d_min -> 0
        assert tuple(e[f * 8, 12 + 2]) == tuple(tab[0]) and tuple(e[f * 8, 24 + 3]) == tuple(tab[255])       # under, over
    assert tuple(e[1, 12 + 2]) == tuple(tab[255]) and tuple(e[8 + 6, 24 + 7]) == tuple(tab[0])               # +Inf, -Inf
    assert (np.asarray(c["B"]["maps"][0]) == 0).sum() == 9


@pytest.mark.parametrize("name", CASES)
def test_emulated_depth_rows_equal_the_restatement(name):
    c = viz_ref.cases()[name]
    L = harness.get_lib("emu")
    n = c["maps"][0].shape[0]
    scratch = torch.full((max(1, L.fd_depth_rows_scratch_bytes(n)),), 0xFF, dtype=torch.uint8)       # (all-ones words are NaNs: nothing may count on zeroed scratch)
    first = run_emu(c["x"], c["maps"], c["value_range"], c["pitch_extra"], scratch)
    check_canvas(first, viz_ref.want(name), name)
    if name != "F":
        again = run_emu(c["x"], c["maps"], c["value_range"], c["pitch_extra"], scratch)               # the same scratch, used
        assert again.tobytes() == first.tobytes(), name


def test_emulated_golden_sample():
    x, d, p = viz_ref.sample()
    check_canvas(run_emu(x, [d, p]), np.load(os.path.join(viz_ref.GOLD, "viz_sample_row.npy")), "sample")


def test_emulated_byte_path_on_dword_sizes():
    """Case B's sizes allow dword stores; a canvas at an odd address, or an odd pitch, takes the byte path and gives the same bytes."""
    c = viz_ref.cases()["B"]
    check_canvas(run_emu(c["x"], c["maps"], misalign=1), viz_ref.want("B"), "B at an odd address")
    check_canvas(run_emu(c["x"], c["maps"], pitch_extra=3), viz_ref.want("B"), "B with an odd pitch")
    check_canvas(run_emu(c["x"], c["maps"], pitch_extra=8), viz_ref.want("B"), "B with a padded pitch, dword path")


def test_nan_frame_leaves_its_neighbours_alone():
    c, clean = viz_ref.cases()["D"], viz_ref.cases()["D_clean"]
    got, base = run_emu(c["x"], c["maps"]), run_emu(clean["x"], clean["maps"])
    assert np.array_equal(got[:8], base[:8]) and np.array_equal(got[16:], base[16:])                  # frames 0 and 2: unchanged
    assert np.array_equal(got[8:16, :36], base[8:16, :36]) and not got[8:16, 36:].any()               # frame 1: colour panel intact, depth panels black


def test_error_paths():
    L = harness.get_lib("emu")
    x, m = torch.rand(1, 3, 4, 8), [torch.rand(1, 1, 4, 8) + 1 for _ in range(3)]
    canvas = torch.zeros(4 * 4 * 8 * 3, dtype=torch.uint8)
    scratch = torch.empty(L.fd_depth_rows_scratch_bytes(1), dtype=torch.uint8)
    rng = torch.tensor([[0.0, 2.0]])

    def call(x=x.data_ptr(), m0=m[0].data_ptr(), m1=m[1].data_ptr(), m2=m[2].data_ptr(), n=1, h=4, w=8, rng=None, canvas=canvas.data_ptr(), pitch=4 * 8 * 3,
             scratch=scratch.data_ptr()):
        rc = L.fd_depth_rows(x, m0, m1, m2, n, h, w, rng, canvas, pitch, scratch, None)
        return rc, L.fd_last_error().decode()

    assert call()[0] == 0
    assert call(x=None, m1=None, m2=None, pitch=8 * 3)[0] == 0
    assert call(scratch=None, rng=rng.data_ptr())[0] == 0                      # no scratch needed when the range is given
    bad = [dict(n=0), dict(h=0), dict(w=-1), dict(m0=None), dict(m1=None), dict(canvas=None), dict(pitch=4 * 8 * 3 - 1), dict(scratch=None)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and "fd_depth_rows" in msg, (kw, rc, msg)
    assert "map2 given without map1" in call(m1=None)[1]
    assert "pitch_bytes" in call(pitch=8 * 3 * 3)[1] and call(x=None, pitch=8 * 3 * 3)[0] == 0
    assert L.fd_depth_rows_scratch_bytes(0) == 0 and L.fd_depth_rows_scratch_bytes(3) >= 3 * 8


def test_paint_rows_shapes_and_canvas_views():
    from fastdepth_hip import viz
    L = harness.get_lib("emu")
    c = viz_ref.cases()["B"]
    x, maps = torch.from_numpy(np.array(c["x"])), [torch.from_numpy(np.array(m)) for m in c["maps"]]
    out = viz.paint_rows(x, *maps, _library=L)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2 * 32, 4 * 36, 3) and np.array_equal(out.numpy(), viz_ref.want("B"))
    out3 = viz.paint_rows(x, *[m[:, 0] for m in maps], _library=L)             # [n, h, w] maps
    assert torch.equal(out3, out)
    one = viz.paint_rows(x[1], *[m[1, 0] for m in maps], _library=L)           # one frame: [3, h, w] and [h, w]
    assert torch.equal(one, out[32:])
    wide = torch.full((2 * 32, 4 * 36 + 5, 3), PREFILL, dtype=torch.uint8)     # a view into a wider canvas
    assert viz.paint_rows(x, *maps, out=wide[:, 2:2 + 4 * 36], _library=L).data_ptr() == wide[:, 2:].data_ptr()
    assert torch.equal(wide[:, 2:2 + 4 * 36], out) and (wide[:, :2] == PREFILL).all() and (wide[:, 2 + 4 * 36:] == PREFILL).all()
    e = viz_ref.cases()["E"]
    got = viz.paint_rows(torch.from_numpy(np.array(e["x"])), *[torch.from_numpy(np.array(m)) for m in e["maps"]], value_range=np.array(e["value_range"]), _library=L)
    assert np.array_equal(got.numpy(), viz_ref.want("E"))
    pair = viz.paint_rows(None, maps[0], value_range=(1.0, 9.0), _library=L)   # one pair for all frames
    assert np.array_equal(pair.numpy(), viz_ref.paint_rows(None, [c["maps"][0]], np.array([[1.0, 9.0]] * 2, np.float32)))
    with pytest.raises(ValueError):
        viz.paint_rows(x, _library=L)
    with pytest.raises(ValueError):
        viz.paint_rows(x, maps[0][:1], _library=L)
    with pytest.raises(ValueError):
        viz.paint_rows(x, *maps, out=torch.zeros(2 * 32, 4 * 36 - 1, 3, dtype=torch.uint8), _library=L)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        viz.paint_rows(x, *maps)


def test_png_writer_round_trips(tmp_path):
    from fastdepth_hip import viz
    img = np.array(viz_ref.want("B"))
    data = viz.encode_png(img)
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (img.shape[1], img.shape[0])
    assert np.array_equal(viz_ref.png_decode(data), img)
    assert viz.encode_png(torch.from_numpy(img)) == data
    path = str(tmp_path / "row.png")
    viz.save_png(img, path)
    assert open(path, "rb").read() == data
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
    with pytest.raises(ValueError):
        viz.encode_png(img.astype(np.float32))
    one = np.array([[[1, 2, 3]]], np.uint8)
    assert np.array_equal(viz_ref.png_decode(viz.encode_png(one)), one)
    assert zlib.crc32(b"IEND") & 0xffffffff == struct.unpack(">I", data[-4:])[0]


def test_utils_surface(tmp_path):
    import utils
    L = harness.get_lib("emu")
    x, d, p = viz_ref.sample()
    gold = np.load(os.path.join(viz_ref.GOLD, "viz_sample_row.npy"))
    row = utils.merge_into_row(torch.from_numpy(x), torch.from_numpy(d), torch.from_numpy(p), _library=L)
    assert isinstance(row, np.ndarray) and row.dtype == np.uint8 and np.array_equal(row, gold)
    assert np.array_equal(utils.merge_into_row(x, d[0, 0], p[0], _library=L), gold)                 # NumPy inputs, squeezed forms
    four = utils.merge_into_row_with_gt(x, d, d, p, _library=L)
    assert four.shape == (224, 4 * 224, 3) and four.dtype == np.uint8
    assert np.array_equal(four[:, :448], gold[:, :448]) and np.array_equal(four[:, 448:], gold[:, 224:])
    col = utils.colored_depthmap(d[0, 0], _library=L)
    lo, hi = viz_ref.frame_range([d[0, 0]])
    assert col.shape == (224, 224, 3) and col.dtype == np.uint8 and np.array_equal(col, viz_ref.colour(d[0, 0], lo, hi))
    assert np.array_equal(utils.colored_depthmap(d[0, 0], 0.0, 10.0, _library=L), viz_ref.colour(d[0, 0], 0.0, 10.0))
    assert np.array_equal(utils.colored_depthmap(d[0, 0], d_max=12.0, _library=L), viz_ref.colour(d[0, 0], lo, 12.0))
    both = utils.add_row(row, row.astype(np.float64))                                                 # either form stacks
    assert both.shape == (448, 672, 3) and both.dtype == np.uint8 and np.array_equal(both[:224], gold) and np.array_equal(both[224:], gold)
    path = str(tmp_path / "comparison.png")
    utils.save_image(both, path)
    pixels = viz_ref.png_decode(open(path, "rb").read())
    assert np.array_equal(pixels, both)
    try:
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), both)
    except ImportError:
        pass
    utils.save_image(both.astype(np.float64), path)                                                   # the reference's float image
    assert np.array_equal(viz_ref.png_decode(open(path, "rb").read()), both)
    args = utils.parse_command(["--comparison", "c.png", "--comparison-skip", "7"])
    assert args.comparison == "c.png" and args.comparison_skip == 7 and args.print_freq == 50
    plain = utils.parse_command([])
    assert plain.comparison == "" and plain.comparison_skip == 50


def test_comparison_frame_selection():
    """evaluate.validate needs the device (the model's forward has no CPU path), so the CPU tier checks the helper that picks the frames: which frames
    of a batch go into which row.  5 frames, skip 2, batch size 2: frames 0, 2, 4 in three batches; batch size 3 puts them at positions 0, 2, 1."""
    import evaluate
    sel = evaluate.comparison_frames
    assert [sel(s, c, 2) for s, c in ((0, 2), (2, 2), (4, 1))] == [[(0, 0)], [(0, 1)], [(0, 2)]]
    assert [sel(s, c, 2) for s, c in ((0, 3), (3, 2))] == [[(0, 0), (2, 1)], [(1, 2)]]
    assert sel(0, 32, 50) == [(0, 0)] and sel(32, 32, 50) == [(18, 1)] and sel(64, 32, 50) == []
    assert sel(0, 1000, 50) == [(50 * r, r) for r in range(8)]                                        # never more than 8 rows
    assert sel(384, 32, 50) == [] and sel(0, 5, 1) == [(r, r) for r in range(5)]
    got = []
    for start in range(0, 403, 7):                                                                    # any batching gives the same frames
        got += [(start + pos, row) for pos, row in sel(start, min(7, 403 - start), 50)]
    assert got == [(50 * r, r) for r in range(8)]
    with pytest.raises(ValueError):
        sel(0, 4, 0)
