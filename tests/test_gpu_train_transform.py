"""The training augmentation on a real MI355X: GpuTrainTransform == the NumPy index-map / float32-blend restatement
(tests/train_transform_ref.py, form (b): neither PIL nor SciPy needed) bit for bit at B = 32 on raw 480 x 640 frames -- which is what FMA
contraction of the rotation or of PIL's blend, or a division that is not IEEE, would break -- and an augmented batch through TrainEngine.step."""
import copy

import numpy as np
import pytest
import torch

import harness
import train_transform_ref as ref
from dataloaders import nyu
from fastdepth_hip import capi
from oracle import inputs

pytestmark = pytest.mark.gpu

B = 32


def test_gpu_train_transform_equals_numpy_form():
    params = ref.coverage_params(B)
    rgb, depth = ref.coverage_frames(B)
    want = [ref.train_transform_numpy(rgb[f], depth[f], p) for f, p in enumerate(params)]
    for f in (0, 1):                                       # s = 1.0, angle = +-5: the out-of-frame path is really taken
        assert int((want[f][1] == 0).sum()) > 0, f
    t = nyu.GpuTrainTransform((224, 224), "cuda")
    rgb_g, depth_g = torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda()
    rec = ref.to_records(params, nyu.AUG_DTYPE)
    x, d = t(rgb_g, depth_g, rec)
    assert x.shape == (B, 3, 224, 224) and d.shape == (B, 1, 224, 224)
    x, d = x.permute(0, 2, 3, 1).cpu().numpy(), d[:, 0].cpu().numpy()
    for f in range(B):
        wx = want[f][0].astype(np.float32)
        assert np.array_equal(x[f], wx), (f, params[f], int((x[f] != wx).sum()))
        assert np.array_equal(d[f], want[f][1]), (f, params[f], int((d[f] != want[f][1]).sum()))
    # repeatable, and the same colour frames without a depth map
    x2, d2 = t(rgb_g, depth_g, rec)
    assert np.array_equal(x2.permute(0, 2, 3, 1).cpu().numpy(), x) and np.array_equal(d2[:, 0].cpu().numpy(), d)
    x3 = t(rgb_g, None, rec)
    assert np.array_equal(x3.permute(0, 2, 3, 1).cpu().numpy(), x)


def test_gpu_train_transform_samples_its_own_parameters():
    """params=None: the transform draws from its generator in the reference's order -- the same seed, the same augmentation."""
    rgb, depth = ref.coverage_frames(4)
    t = nyu.GpuTrainTransform((224, 224), "cuda", rng=np.random.RandomState(5))
    x, d = t(torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda())
    rec = nyu.sample_train_params(4, np.random.RandomState(5))
    for f in range(4):
        wx, wd = ref.train_transform_numpy(rgb[f], depth[f], ref.from_record(rec[f]))
        assert np.array_equal(x[f].permute(1, 2, 0).cpu().numpy(), wx.astype(np.float32)) and np.array_equal(d[f, 0].cpu().numpy(), wd), f
    with pytest.raises(ValueError, match="permutation"):
        bad = rec.copy(); bad["order"][0] = (1, 1, 1)
        t(torch.from_numpy(rgb).cuda(), None, bad)


def test_record_refused_on_the_device_gives_a_zero_frame():
    """Records in device memory are checked by the table step (nothing synchronises): a refused frame is all zeros -- depth 0 is 'invalid', so the
    masked loss ignores it -- and its neighbours are untouched."""
    L = harness.get_lib("hip")
    rgb, depth = ref.coverage_frames(4)
    params = ref.coverage_params(14)[4:7]
    rec = ref.to_records(params, nyu.AUG_DTYPE)
    rec["order"][1] = (7, -3, 7)
    rec["s"][2] = 0.5
    rgb_g, depth_g = torch.from_numpy(rgb[:3]).cuda(), torch.from_numpy(depth[:3]).cuda()
    p_g = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    x, d = torch.full((3, 3, 224, 224), float("nan"), device="cuda"), torch.full((3, 1, 224, 224), float("nan"), device="cuda")
    scratch = torch.empty(L.fd_train_transform_scratch_bytes(3, 224, 224), dtype=torch.uint8, device="cuda")
    capi.check(L, L.fd_train_transform(rgb_g.data_ptr(), depth_g.data_ptr(), 3, 480, 640, 224, 224, p_g.data_ptr(), x.data_ptr(), d.data_ptr(),
                                       scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "fd_train_transform")
    torch.cuda.synchronize()
    wx, wd = ref.train_transform_numpy(rgb[0], depth[0], params[0])
    assert np.array_equal(x[0].permute(1, 2, 0).cpu().numpy(), wx.astype(np.float32)) and np.array_equal(d[0, 0].cpu().numpy(), wd)
    for f in (1, 2):
        assert float(x[f].abs().max()) == 0.0 and float(d[f].abs().max()) == 0.0, f


def test_train_step_on_an_augmented_batch():
    """One TrainEngine.step (bf16 plan, masked L1: rotated-out pixels carry depth 0) on an augmented batch: a finite loss, and a second identical
    run -- transform and step -- gives the same bits."""
    from fastdepth_hip.train import TrainEngine
    models = inputs.product_models()
    torch.manual_seed(3)
    m0 = models.MobileNetSkipAdd((224, 224), pretrained=False)
    m0.decode_conv6[1].bias.data.fill_(2.8)
    rgb, depth = ref.coverage_frames(B)
    rec = ref.to_records(ref.coverage_params(B), nyu.AUG_DTYPE)
    rgb_g, depth_g = torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda()
    out = []
    for _ in range(2):
        m = copy.deepcopy(m0).cuda().train()
        eng = TrainEngine(m, lr=0.01, dtype=torch.bfloat16, masked_loss=True)
        x, d = nyu.GpuTrainTransform((224, 224), "cuda")(rgb_g, depth_g, rec)
        assert int((d == 0).sum()) > 0                    # the mask has something to do
        loss = eng.step(x, d)
        torch.cuda.synchronize()
        out.append((loss.detach().cpu().clone(), m.conv0[0].weight.detach().cpu().clone()))
    assert torch.isfinite(out[0][0]).all(), out[0][0]
    assert out[0][0].numpy().tobytes() == out[1][0].numpy().tobytes()
    assert out[0][1].numpy().tobytes() == out[1][1].numpy().tobytes()
