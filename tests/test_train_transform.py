"""The training augmentation (reference dataloaders/nyu.py:26-46 train_transform) on the CPU tier: the two restatements in
tests/train_transform_ref.py agree with each other, and fd_train_transform -- its kernels compiled for the emulator -- agrees with the PIL + SciPy
form bit for bit; the random stream; the error paths."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import harness
import train_transform_ref as ref
from dataloaders import nyu
from fastdepth_hip import capi

OUT = (224, 224)


def run_emu(rgb, depth, rec, out=OUT):
    """fd_train_transform of the emulator build on NumPy inputs -> (x [n, oh, ow, 3] float32, depth [n, oh, ow] float32 or None)."""
    L = harness.get_lib("emu")
    n, H, W = rgb.shape[:3]
    rgb_t, rec_t = torch.from_numpy(np.ascontiguousarray(rgb)), torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy())
    x = torch.full((n, 3) + out, float("nan"))
    d_in = torch.from_numpy(np.ascontiguousarray(depth)) if depth is not None else None
    d = torch.full((n, 1) + out, float("nan")) if depth is not None else None
    nbytes = L.fd_train_transform_scratch_bytes(n, *out)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 128, dtype=torch.uint8)
    base = (scratch.data_ptr() + 127) // 128 * 128
    capi.check(L, L.fd_train_transform(rgb_t.data_ptr(), d_in.data_ptr() if d_in is not None else None, n, H, W, out[0], out[1], rec_t.data_ptr(),
                                       x.data_ptr(), d.data_ptr() if d is not None else None, base, None), "fd_train_transform")
    return x.permute(0, 2, 3, 1).contiguous().numpy(), (d[:, 0].numpy() if d is not None else None)


def test_record_layout_matches_the_header():
    assert nyu.AUG_DTYPE.itemsize == ctypes.sizeof(capi.AugParams) == 48
    for name in nyu.AUG_DTYPE.names:
        assert nyu.AUG_DTYPE.fields[name][1] == getattr(capi.AugParams, name).offset, name


def test_pil_form_equals_numpy_form():
    """(a) PIL + SciPy == (b) index map + float32 blends, exactly, on random raw-size frames (and on the uniform and the dark one)."""
    params = ref.coverage_params(14)
    rgb, depth = ref.coverage_frames(14)
    for f, p in enumerate(params):
        xa, da = ref.train_transform_pil(rgb[f], depth[f], p)
        xb, db = ref.train_transform_numpy(rgb[f], depth[f], p)
        assert np.array_equal(xa, xb), (f, p, int((xa != xb).sum()))
        assert np.array_equal(da, db), (f, p, int((da != db).sum()))


def test_emulated_train_transform_equals_pil_and_scipy():
    """fd_train_transform (emulator build) == the PIL + SciPy restatement: x and depth bit for bit, every frame, every pixel."""
    n = 14
    params = ref.coverage_params(n)
    rgb, depth = ref.coverage_frames(n)
    want = [ref.train_transform_pil(rgb[f], depth[f], p) for f, p in enumerate(params)]
    for f in (0, 1):                                       # s = 1.0, angle = +-5: the out-of-frame path is really taken
        assert int((want[f][1] == 0).sum()) > 0, f
    assert all(int((want[f][1] == 0).sum()) == 0 for f in range(n) if params[f]["angle"] == 0.0)
    x, d = run_emu(rgb, depth, ref.to_records(params, nyu.AUG_DTYPE))
    for f in range(n):
        assert np.array_equal(x[f], want[f][0].astype(np.float32)), (f, params[f], int((x[f] != want[f][0].astype(np.float32)).sum()))
        assert np.array_equal(d[f], want[f][1]), (f, params[f], int((d[f] != want[f][1]).sum()))
    # without a depth map: the same colour frames
    x2, d2 = run_emu(rgb[:4], None, ref.to_records(params[:4], nyu.AUG_DTYPE))
    assert d2 is None and np.array_equal(x2, x[:4])


def test_emulated_train_transform_other_output_size():
    """A non-square output that is no multiple of the workgroup's pixel count: the tail of the gather / apply loops and the column tables."""
    params = ref.coverage_params(14)[:3]
    rgb, depth = ref.coverage_frames(4)
    x, d = run_emu(rgb[:3], depth[:3], ref.to_records(params, nyu.AUG_DTYPE), out=(96, 131))
    for f, p in enumerate(params):
        wx, wd = ref.train_transform_pil(rgb[f], depth[f], p, output_size=(96, 131))
        assert np.array_equal(x[f], wx.astype(np.float32)) and np.array_equal(d[f], wd), f


def test_emulated_train_transform_is_repeatable():
    params = ref.coverage_params(14)[:6]
    rgb, depth = ref.coverage_frames(6)
    rec = ref.to_records(params, nyu.AUG_DTYPE)
    x1, d1 = run_emu(rgb, depth, rec)
    x2, d2 = run_emu(rgb, depth, rec)
    assert x1.tobytes() == x2.tobytes() and d1.tobytes() == d2.tobytes()
    assert not np.isnan(x1).any() and not np.isnan(d1).any()


@pytest.mark.parametrize("seed", [0, 1, 7, 2024])
def test_sampled_parameters_follow_the_reference_stream(seed):
    rec = nyu.sample_train_params(5, np.random.RandomState(seed))
    np.random.seed(seed)
    want = ref.draw_params(5)
    for r, p in zip(rec, want):
        assert r["s"] == p["s"] and r["angle"] == p["angle"] and bool(r["flip"]) == p["flip"]
        for k in ("brightness", "contrast", "saturation"):
            assert r[k] == np.float32(p[k])
        assert tuple(r["order"]) == p["order"]
        assert 1.0 <= r["s"] <= 1.5 and -5.0 <= r["angle"] <= 5.0
    nyu.check_train_params(rec, 5)


_REFERENCE_RUN = r"""
import sys, types, collections, collections.abc
sys.dont_write_bytecode = True
import numpy as np
ref_root, tests_dir, seed, src, dst = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
sys.path.insert(0, tests_dir)
import train_transform_ref as R
collections.Iterable = collections.abc.Iterable                      # removed in Python 3.10
np.asfarray = lambda a, dtype=float: np.asarray(a, dtype=np.float64)   # removed in NumPy 2
sys.modules["h5py"] = types.ModuleType("h5py")                       # only the file loader needs it
import scipy, scipy.ndimage
misc = types.ModuleType("scipy.misc")                                # removed in SciPy 1.12; imresize in 1.3
misc.imresize = lambda arr, size, interp="nearest", mode=None: R._imresize(arr, size, mode)
sys.modules["scipy.misc"] = misc; scipy.misc = misc
try:
    import scipy.ndimage.interpolation                               # a deprecated alias of scipy.ndimage
except Exception:
    sys.modules["scipy.ndimage.interpolation"] = scipy.ndimage
sys.path.insert(0, ref_root)
from dataloaders.nyu import NYUDataset
ds = NYUDataset.__new__(NYUDataset)                                  # (the constructor walks a dataset directory)
ds.output_size = (224, 224)
z = np.load(src)
np.random.seed(seed)
xs, ds_ = [], []
for f in range(len(z["rgb"])):
    x, d = ds.train_transform(z["rgb"][f], z["depth"][f])
    xs.append(x); ds_.append(d)
np.savez(dst, x=np.stack(xs), d=np.stack(ds_))
"""


def test_reference_train_transform_itself_under_the_same_seed(tmp_path):
    """The reference's own NYUDataset.train_transform (when its tree is present), run in a child process with the APIs it needs and that have since
    been removed shimmed there, under seed k == the PIL + SciPy restatement with sample_train_params(n, RandomState(k))."""
    root = os.environ.get("FD_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(root, "dataloaders", "nyu.py")):
        pytest.skip("reference tree not present")
    rgb, depth = ref.coverage_frames(4)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, rgb=rgb, depth=depth)
    seed = 11
    subprocess.run([sys.executable, "-c", _REFERENCE_RUN, root, os.path.dirname(os.path.abspath(__file__)), str(seed), src, dst], check=True)
    got = np.load(dst)
    rec = nyu.sample_train_params(4, np.random.RandomState(seed))
    for f, r in enumerate(rec):
        p = ref.from_record(r)
        wx, wd = ref.train_transform_pil(rgb[f], depth[f], p)
        assert np.array_equal(got["x"][f], wx) and np.array_equal(got["d"][f], wd), f


def test_error_paths():
    L = harness.get_lib("emu")
    rgb, depth = ref.coverage_frames(4, 480, 640)
    rgb, depth = rgb[:1], depth[:1]
    good = ref.coverage_params(14)[4]

    def call(rgb=rgb, depth=depth, p=good, with_depth_out=True, H=480, W=640, n=1, null=None):
        rec = ref.to_records([p], nyu.AUG_DTYPE)
        r_t, d_t, p_t = torch.from_numpy(rgb), torch.from_numpy(depth) if depth is not None else None, torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
        x, d = torch.zeros(1, 3, 224, 224), torch.zeros(1, 1, 224, 224)
        scratch = torch.empty(L.fd_train_transform_scratch_bytes(1, 224, 224) + 128, dtype=torch.uint8)
        args = dict(rgb=r_t.data_ptr(), depth=d_t.data_ptr() if d_t is not None else None, params=p_t.data_ptr(), x=x.data_ptr(),
                    d=d.data_ptr() if with_depth_out else None, scratch=(scratch.data_ptr() + 127) // 128 * 128)
        if null:
            args[null] = None
        rc = L.fd_train_transform(args["rgb"], args["depth"], n, H, W, 224, 224, args["params"], args["x"], args["d"], args["scratch"], None)
        return rc, L.fd_last_error().decode()

    assert call()[0] == 0
    for null in ("rgb", "params", "x", "scratch"):
        rc, msg = call(null=null)
        assert rc == -1 and "null/empty" in msg, (null, rc, msg)
    rc, msg = call(n=0)
    assert rc == -1 and "null/empty" in msg
    assert L.fd_train_transform_scratch_bytes(0, 224, 224) == 0
    for kw in (dict(with_depth_out=False), dict(depth=None)):
        rc, msg = call(**kw)
        assert rc == -1 and "go together" in msg, (kw, msg)
    for order in ((0, 0, 1), (0, 1, 3), (-1, 1, 2)):
        rc, msg = call(p=dict(good, order=order))
        assert rc == -1 and "permutation" in msg, (order, msg)
    rc, msg = call(p=dict(good, s=0.9))                 # 250 x 333 -> 225 x 299 < 228 x 304
    assert rc == -1 and "smaller than the 228 x 304 crop" in msg, msg
    for s in (float("nan"), 0.0, 1e9):
        rc, msg = call(p=dict(good, s=s))
        assert rc == -1 and "is not in" in msg, (s, msg)
    for k, v in (("brightness", float("nan")), ("contrast", float("inf")), ("saturation", float("-inf")), ("angle", float("nan"))):
        rc, msg = call(p=dict(good, **{k: v}))
        assert rc == -1 and "not finite" in msg, (k, v, msg)
    small = np.zeros((1, 100, 20, 3), np.uint8)         # resizes to 250 x 50: no scale the library admits (s <= 4) reaches 304 columns
    rc, msg = call(rgb=small, depth=np.ones((1, 100, 20), np.float32), H=100, W=20)
    assert rc == -1 and "too small" in msg, msg


def test_python_side_refuses_bad_records():
    """GpuTrainTransform checks the records on the host before the upload (records in device memory are checked by the device only)."""
    rec = nyu.sample_train_params(3, np.random.RandomState(0))
    nyu.check_train_params(rec, 3)
    bad = rec.copy(); bad["order"][1] = (0, 0, 2)
    with pytest.raises(ValueError, match="permutation"):
        nyu.check_train_params(bad, 3)
    bad = rec.copy(); bad["s"][2] = 0.5
    with pytest.raises(ValueError, match="crop"):
        nyu.check_train_params(bad, 3)
    bad = rec.copy(); bad["contrast"][0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        nyu.check_train_params(bad, 3)
    with pytest.raises(ValueError, match="records"):
        nyu.check_train_params(rec, 4)
