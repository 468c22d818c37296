"""NYU-Depth-v2 validation transform and training augmentation on the GPU.

Reference: dataloaders/nyu.py:5 (raw frames are 480 x 640), :48-59 `val_transform`
    Resize(250.0 / iheight) -> CenterCrop((228, 304)) -> Resize(output_size)      (transforms.py:311-341, 344-392)
followed by `/ 255` for the colour image; every Resize is scipy.misc.imresize(..., 'nearest'), i.e. PIL's NEAREST resize.
Nearest-neighbour resizing and cropping are index maps, so the whole chain is one row table and one column table; the tables
reproduce PIL's arithmetic exactly (its affine scaler accumulates the source coordinate by repeated addition in double and
truncates: x_src[i] = int(s/2 + s + s + ...), pinned against PIL itself by tests/test_oracle.py).  `GpuValTransform` uploads
the tables once and calls `fd_val_transform`, which gathers raw uint8 HWC frames (+ raw depth) into the network's NCHW float
input (+ the depth target) -- no per-frame CPU work.

Training: dataloaders/nyu.py:26-46 `train_transform` draws a scale s in [1, 1.5], an angle in [-5, 5] degrees and a flip per frame, runs
    Resize(250.0 / iheight) -> Rotate(angle) -> Resize(s) -> CenterCrop((228, 304)) -> HorizontalFlip -> Resize(output_size)
on the colour frame and on depth / s, and applies ColorJitter(0.4, 0.4, 0.4) (dataloader.py:46, transforms.py:513-578: PIL's Brightness /
Contrast / Color enhancers in a shuffled order) to the colour frame.  Rotate is scipy.ndimage.rotate(order=0, reshape=False): nearest-neighbour
again, so the geometry is one per-frame index map with zeros where the rotation leaves the frame, and PIL's enhancers are float32 blends of uint8
images.  `sample_train_params` draws the parameters in the reference's order (the same seed gives the same augmentations); `GpuTrainTransform`
uploads the n parameter records and calls `fd_train_transform`, which builds the per-frame tables on the device and reproduces the chain bit for
bit -- as PIL 12 and SciPy 1.15 compute it (tests/train_transform_ref.py): in that SciPy a rotated sample is inside iff its source coordinate lies
in [0, n - 1]; the SciPy of the reference's era (< 1.3, it still had scipy.misc.imresize) may have drawn single border pixels of a rotated frame
differently.  Rotated-out pixels carry depth 0, i.e. "invalid": train with the masked L1 loss (TrainEngine(masked_loss=True)).
"""
import numpy as np
import torch

IHEIGHT, IWIDTH = 480, 640           # raw NYU frame (reference nyu.py:5)


def _nearest_table(n_in, n_out):
    """Source index of every output index for PIL's NEAREST resize of n_in samples to n_out."""
    scale = n_in / n_out
    pos, tab = scale * 0.5, np.empty(n_out, np.int32)
    for i in range(n_out):
        tab[i] = int(pos)
        pos += scale
    return np.minimum(tab, n_in - 1)


def val_index_maps(output_size=(224, 224), iheight=IHEIGHT, iwidth=IWIDTH):
    """(ymap[out_h], xmap[out_w]): raw-frame row / column read by each output row / column."""
    f = 250.0 / iheight
    w1, h1 = int(iwidth * f), int(iheight * f)                 # imresize with a float: size = (array(im.size) * f).astype(int)
    y1, x1 = _nearest_table(iheight, h1), _nearest_table(iwidth, w1)
    th, tw = 228, 304
    i, j = int(round((h1 - th) / 2.)), int(round((w1 - tw) / 2.))     # CenterCrop.get_params (transforms.py:373-374)
    if i < 0 or j < 0:
        raise ValueError("frame too small for the 228 x 304 centre crop")
    oh, ow = output_size
    y2, x2 = _nearest_table(th, oh), _nearest_table(tw, ow)
    return y1[i + y2].astype(np.int32), x1[j + x2].astype(np.int32)


class GpuValTransform:
    """rgb [n, H, W, 3] uint8 (GPU), depth [n, H, W] float32 (GPU, optional) -> x [n, 3, oh, ow] float32, depth [n, 1, oh, ow]."""

    def __init__(self, output_size=(224, 224), device="cuda", iheight=IHEIGHT, iwidth=IWIDTH):
        self.output_size, self.raw = tuple(output_size), (iheight, iwidth)
        ymap, xmap = val_index_maps(output_size, iheight, iwidth)
        self.ymap, self.xmap = torch.from_numpy(ymap).to(device), torch.from_numpy(xmap).to(device)

    def __call__(self, rgb, depth=None):
        from fastdepth_hip import capi
        from fastdepth_hip.engine import lib
        if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[-1] != 3 or tuple(rgb.shape[1:3]) != self.raw:
            raise RuntimeError("expected a uint8 [n, %d, %d, 3] GPU tensor, got %s %s on %s" % (self.raw + (tuple(rgb.shape), rgb.dtype, rgb.device)))
        rgb = rgb.contiguous()
        n, (oh, ow) = rgb.shape[0], self.output_size
        x = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=rgb.device)
        d = dp = None
        if depth is not None:
            if not depth.is_cuda or depth.dtype != torch.float32 or tuple(depth.shape) != (n,) + self.raw:
                raise RuntimeError("expected a float32 [n, %d, %d] GPU depth tensor" % self.raw)
            depth = depth.contiguous()
            d = torch.empty((n, 1, oh, ow), dtype=torch.float32, device=rgb.device)
            dp = depth.data_ptr()
        L = lib()
        with torch.cuda.device(rgb.device):
            capi.check(L, L.fd_val_transform(rgb.data_ptr(), dp, n, self.raw[0], self.raw[1], oh, ow, self.ymap.data_ptr(), self.xmap.data_ptr(),
                                             x.data_ptr(), d.data_ptr() if d is not None else None,
                                             torch.cuda.current_stream(rgb.device).cuda_stream), "fd_val_transform")
        return (x, d) if depth is not None else x


# fd_aug_params (include/fastdepth_hip.h) as a NumPy record: one frame's augmentation
AUG_DTYPE = np.dtype([("s", "<f8"), ("angle", "<f8"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("flip", "<i4"),
                      ("order", "<i4", (3,)), ("reserved", "<i4")])
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2      # the entries of `order`
MAX_SCALE = 4.0                                 # FD_AUG_MAX_SCALE (csrc/fd_kernels_io.h)


def sample_train_params(n, rng=np.random):
    """n records of AUG_DTYPE drawn from `rng` (numpy.random or a RandomState) exactly as the reference draws them, frame after frame: s, angle,
    flip (nyu.py:27-30), then ColorJitter.get_params(0.4, 0.4, 0.4): brightness, contrast, saturation factors and the shuffle of the three ops
    (transforms.py:542-560)."""
    rec = np.zeros(n, AUG_DTYPE)
    for r in rec:
        r["s"] = rng.uniform(1.0, 1.5)
        r["angle"] = rng.uniform(-5.0, 5.0)
        r["flip"] = rng.uniform(0.0, 1.0) < 0.5
        for name in ("brightness", "contrast", "saturation"):
            r[name] = rng.uniform(0.6, 1.4)                # max(0, 1 - 0.4), 1 + 0.4; PIL receives the factor as a C float
        order = [BRIGHTNESS, CONTRAST, SATURATION]
        rng.shuffle(order)
        r["order"] = order
    return rec


def check_train_params(params, n, iheight=IHEIGHT, iwidth=IWIDTH):
    """What fd_train_transform requires of the records (the library checks records in device memory on the device only: csrc/fd_kernels_io.h)."""
    params = np.ascontiguousarray(params)
    if params.dtype != AUG_DTYPE or params.shape != (n,):
        raise ValueError("expected %d records of AUG_DTYPE, got %s %s" % (n, params.shape, params.dtype))
    if not (np.sort(params["order"], axis=1) == np.arange(3)).all():
        raise ValueError("order must be a permutation of (0, 1, 2) in every record")
    s = params["s"]
    if not ((s > 0) & (s <= MAX_SCALE)).all():
        raise ValueError("s must lie in (0, %g]" % MAX_SCALE)
    if not all(np.isfinite(params[k]).all() for k in ("angle", "brightness", "contrast", "saturation")):
        raise ValueError("angle and the colour factors must be finite")
    f = 250.0 / iheight
    h1, w1 = int(iheight * f), int(iwidth * f)
    if ((h1 * s).astype(int) < 228).any() or ((w1 * s).astype(int) < 304).any():
        raise ValueError("s = %g resizes the %d x %d image below the 228 x 304 crop" % (s.min(), h1, w1))
    return params


class GpuTrainTransform:
    """rgb [n, H, W, 3] uint8 (GPU), depth [n, H, W] float32 (GPU, optional), params: n AUG_DTYPE records (default: sample_train_params(n))
    -> x [n, 3, oh, ow] float32, depth [n, 1, oh, ow] (0 where the rotation left the frame)."""

    def __init__(self, output_size=(224, 224), device="cuda", iheight=IHEIGHT, iwidth=IWIDTH, rng=np.random):
        self.output_size, self.raw, self.device, self.rng = tuple(output_size), (iheight, iwidth), torch.device(device), rng
        self._scratch = None

    def __call__(self, rgb, depth=None, params=None):
        from fastdepth_hip import capi
        from fastdepth_hip.engine import lib
        if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[-1] != 3 or tuple(rgb.shape[1:3]) != self.raw:
            raise RuntimeError("expected a uint8 [n, %d, %d, 3] GPU tensor, got %s %s on %s" % (self.raw + (tuple(rgb.shape), rgb.dtype, rgb.device)))
        rgb = rgb.contiguous()
        n, (oh, ow) = rgb.shape[0], self.output_size
        params = check_train_params(sample_train_params(n, self.rng) if params is None else params, n, *self.raw)
        x = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=rgb.device)
        d = dp = None
        if depth is not None:
            if not depth.is_cuda or depth.dtype != torch.float32 or tuple(depth.shape) != (n,) + self.raw:
                raise RuntimeError("expected a float32 [n, %d, %d] GPU depth tensor" % self.raw)
            depth = depth.contiguous()
            d = torch.empty((n, 1, oh, ow), dtype=torch.float32, device=rgb.device)
            dp = depth.data_ptr()
        L = lib()
        with torch.cuda.device(rgb.device):
            need = L.fd_train_transform_scratch_bytes(n, oh, ow)
            if self._scratch is None or self._scratch.numel() < need or self._scratch.device != rgb.device:
                self._scratch = torch.empty(need, dtype=torch.uint8, device=rgb.device)        # (the caching allocator aligns to 512 bytes)
            # the one upload of the call: n 48-byte records, on the current stream like the kernels that read them
            p_dev = torch.from_numpy(params.view(np.uint8).reshape(-1)).to(rgb.device, non_blocking=True)
            capi.check(L, L.fd_train_transform(rgb.data_ptr(), dp, n, self.raw[0], self.raw[1], oh, ow, p_dev.data_ptr(), x.data_ptr(),
                                               d.data_ptr() if d is not None else None, self._scratch.data_ptr(),
                                               torch.cuda.current_stream(rgb.device).cuda_stream), "fd_train_transform")
        return (x, d) if depth is not None else x
