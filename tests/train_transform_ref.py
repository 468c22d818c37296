"""Restatements of the reference's NYU training augmentation (parity yard-sticks).  TEST INFRASTRUCTURE ONLY.

The reference: dataloaders/nyu.py:26-46 (`train_transform`) draws s, angle, flip (:27-30), runs
    Resize(250/480) -> Rotate(angle) -> Resize(s) -> CenterCrop((228, 304)) -> HorizontalFlip -> Resize(output_size)      (:33-40)
on the colour frame and on depth / s (:28, :44), applies ColorJitter(0.4, 0.4, 0.4) to the colour frame (:42; dataloader.py:46;
transforms.py:532-578) and divides it by 255 (:43).  Two forms of it live here, both with EXPLICIT parameters:

  (a) `train_transform_pil`    the chain step by step on the installed PIL and SciPy, the way oracle/val_transform.py restates the
                               validation chain: Resize is scipy.misc.imresize(..., 'nearest') == PIL's NEAREST resize (transforms.py:329-341),
                               Rotate is scipy.ndimage.rotate(order=0, reshape=False, prefilter=False) (transforms.py:298-308), the colour ops are
                               PIL.ImageEnhance.Brightness / Contrast / Color (transforms.py:34-91).
  (b) `train_transform_numpy`  the same as one index map + float32 blends in NumPy alone (what the device kernels compute, and what the GPU tier
                               compares against: it needs neither PIL nor SciPy).

Pinned against PIL 12 / SciPy 1.15.  In that SciPy a rotated sample is inside the frame iff its source COORDINATE lies in [0, n - 1] on both axes
(mode='constant': half a pixel beyond the outermost sample centres is already outside, although its nearest sample exists); the sample is then the
one at floor(coordinate + 0.5).  The SciPy of the reference's era (scipy.misc.imresize still existed: < 1.3) may have drawn that border differently,
so single border pixels of a rotated frame may differ from what that installation produced.  SciPy takes cos / sin from scipy.special.cosdg / sindg; (b) uses cos(radians(angle)), which can differ in
the last place -- enough to move a sample only if a source coordinate lands within ~1e-13 of a half-integer.

`draw_params` restates the random stream (nyu.py:27-30, transforms.py:542-560) on the global NumPy generator.
"""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2       # the entries of `order`
CROP = (228, 304)


def draw_params(n):
    """n frames' parameters from np.random's global stream, in the reference's order of draws."""
    out = []
    for _ in range(n):
        s = np.random.uniform(1.0, 1.5)                       # nyu.py:27
        angle = np.random.uniform(-5.0, 5.0)                  # nyu.py:29
        flip = np.random.uniform(0.0, 1.0) < 0.5              # nyu.py:30
        fac = [np.random.uniform(max(0, 1 - v), 1 + v) for v in (0.4, 0.4, 0.4)]      # transforms.py:543-553 with dataloader.py:46
        order = [BRIGHTNESS, CONTRAST, SATURATION]
        np.random.shuffle(order)                              # transforms.py:559
        out.append(dict(s=s, angle=angle, flip=bool(flip), brightness=fac[0], contrast=fac[1], saturation=fac[2], order=tuple(order)))
    return out


# ---------------------------------------------------------------------------------------------------------------- (a) PIL + SciPy
def _imresize(arr, size, mode=None):
    from PIL import Image
    im = Image.fromarray(arr.astype(np.float32), mode="F") if mode == "F" else Image.fromarray(arr)
    if isinstance(size, float):
        size = tuple((np.array(im.size) * size).astype(int))
    else:
        size = (size[1], size[0])
    return np.asarray(im.resize(size, resample=Image.NEAREST))


def _resize(img, size):
    return _imresize(img, size) if img.ndim == 3 else _imresize(img, size, "F")


def _center_crop(img, size):
    th, tw = size
    h, w = img.shape[0], img.shape[1]
    i, j = int(round((h - th) / 2.)), int(round((w - tw) / 2.))
    return img[i:i + th, j:j + tw]


def train_transform_pil(rgb_u8, depth, p, output_size=(224, 224), iheight=480):
    """rgb_u8 [H, W, 3] uint8, depth [H, W] float32 or None -> (rgb [oh, ow, 3] float64 in [0, 1], depth [oh, ow] float32 or None)."""
    from PIL import Image, ImageEnhance
    from scipy import ndimage

    def chain(img):
        img = _resize(img, 250.0 / iheight)
        img = ndimage.rotate(img, p["angle"], reshape=False, prefilter=False, order=0)
        img = _center_crop(_resize(img, float(p["s"])), CROP)
        if p["flip"]:
            img = np.fliplr(img)
        return _resize(img, tuple(output_size))

    pil = Image.fromarray(chain(rgb_u8))
    ops = {BRIGHTNESS: (ImageEnhance.Brightness, p["brightness"]), CONTRAST: (ImageEnhance.Contrast, p["contrast"]),
           SATURATION: (ImageEnhance.Color, p["saturation"])}
    for o in p["order"]:
        pil = ops[o][0](pil).enhance(float(ops[o][1]))
    x = np.asarray(np.array(pil), dtype=np.float64) / 255
    d = None
    if depth is not None:
        d = chain(depth.astype(np.float32) / float(p["s"]))           # nyu.py:28: a float32 array over a Python float stays float32
    return x, d


# ---------------------------------------------------------------------------------------------------------------- (b) NumPy alone
def _nearest_table(n_in, n_out):
    """PIL's NEAREST resize: the source coordinate is accumulated by repeated addition in double and truncated."""
    scale = n_in / n_out
    pos, tab = scale * 0.5, np.empty(n_out, np.int64)
    for i in range(n_out):
        tab[i] = int(pos)
        pos += scale
    return np.minimum(tab, n_in - 1)


def index_map(p, H, W, output_size=(224, 224)):
    """(src [oh, ow] flat index into the raw H x W frame, valid [oh, ow]): the geometric chain as one map."""
    f = 250.0 / H
    h1, w1 = int(H * f), int(W * f)
    h2, w2 = int(h1 * float(p["s"])), int(w1 * float(p["s"]))
    i, j = int(round((h2 - CROP[0]) / 2.)), int(round((w2 - CROP[1]) / 2.))
    assert i >= 0 and j >= 0
    oh, ow = output_size
    y3, x3 = _nearest_table(CROP[0], oh), _nearest_table(CROP[1], ow)
    if p["flip"]:
        x3 = CROP[1] - 1 - x3
    ya = _nearest_table(h1, h2)[i + y3].astype(np.float64)[:, None]
    xa = _nearest_table(w1, w2)[j + x3].astype(np.float64)[None, :]
    a = np.radians(np.float64(p["angle"]))
    c, s = np.cos(a), np.sin(a)
    cy, cx = (h1 - 1) / 2, (w1 - 1) / 2
    off_y, off_x = cy - (c * cy + s * cx), cx - (-s * cy + c * cx)
    sy = (off_y + ya * c) + xa * s                  # every product and every sum rounded on its own, in this order
    sx = (off_x + ya * (-s)) + xa * c
    iy, ix = np.floor(sy + 0.5).astype(np.int64), np.floor(sx + 0.5).astype(np.int64)
    valid = (sy >= 0) & (sy <= h1 - 1) & (sx >= 0) & (sx <= w1 - 1)      # SciPy's 'constant' mode: the COORDINATE decides, not the rounded index
    y1, x1 = _nearest_table(H, h1), _nearest_table(W, w1)
    src = y1[np.clip(iy, 0, h1 - 1)] * W + x1[np.clip(ix, 0, w1 - 1)]
    return src, valid


def _luma(img):
    v = img.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def _blend(deg, img, alpha):
    """PIL's blend of uint8 images, deg + alpha * (img - deg), in float32 with separately rounded product and sum."""
    alpha = np.float32(alpha)
    diff = (img.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    t = deg.astype(np.float32) + alpha * diff
    if 0 <= alpha <= 1:
        return t.astype(np.uint8)                   # truncation
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def color_jitter_numpy(img, p):
    for o in p["order"]:
        if o == BRIGHTNESS:
            img = _blend(np.zeros_like(img), img, p["brightness"])
        elif o == CONTRAST:
            L = _luma(img)
            m = int(int(L.sum()) / L.size + 0.5)
            img = _blend(np.full_like(img, m), img, p["contrast"])
        else:
            L = _luma(img).astype(np.uint8)
            img = _blend(np.repeat(L[..., None], 3, axis=-1), img, p["saturation"])
    return img


def train_transform_numpy(rgb_u8, depth, p, output_size=(224, 224)):
    H, W = rgb_u8.shape[:2]
    src, valid = index_map(p, H, W, output_size)
    img = np.where(valid[..., None], rgb_u8.reshape(-1, 3)[src], 0).astype(np.uint8)
    x = color_jitter_numpy(img, p).astype(np.float64) / 255
    d = None
    if depth is not None:
        dd = depth.astype(np.float32) / np.float32(p["s"])
        d = np.where(valid, dd.reshape(-1)[src], np.float32(0)).astype(np.float32)
    return x, d


# ---------------------------------------------------------------------------------------------------------------- the frame set both tiers use
def coverage_params(n, seed=0):
    """n >= 14 parameter sets covering: all six orders, both flips, s in {1.0, just under 1.5, random}, angle in {0, +5, -5, random}, factors at
    0.6, 1.0, 1.4 and random.  Frames 0 and 1 are s = 1.0 with angle +5 / -5: the rotation must take pixels from outside the frame there."""
    import itertools
    rs = np.random.RandomState(seed)
    orders = list(itertools.permutations((BRIGHTNESS, CONTRAST, SATURATION)))
    scales, angles, levels = (1.0, np.nextafter(1.5, 0.0), None), (5.0, -5.0, 0.0, None), (0.6, 1.4, 1.0, None)
    out = []
    for k in range(n):
        s, a = scales[0 if k < 2 else k % 3], angles[k % 4]
        fac = [levels[(k + j) % 4] for j in range(3)]
        out.append(dict(s=rs.uniform(1.0, 1.5) if s is None else s, angle=rs.uniform(-5.0, 5.0) if a is None else a, flip=bool((k // 2) % 2 == 0),
                        brightness=rs.uniform(0.6, 1.4) if fac[0] is None else fac[0], contrast=rs.uniform(0.6, 1.4) if fac[1] is None else fac[1],
                        saturation=rs.uniform(0.6, 1.4) if fac[2] is None else fac[2], order=orders[k % 6]))
    assert n >= 14 and {p["order"] for p in out} == set(orders) and {p["flip"] for p in out} == {False, True}
    assert out[0]["s"] == 1.0 and out[0]["angle"] == 5.0 and out[1]["s"] == 1.0 and out[1]["angle"] == -5.0
    return out


def coverage_frames(n, H=480, W=640, seed=1):
    """rgb [n, H, W, 3] uint8 and depth [n, H, W] float32 >= 0.5 (so that a zero in the transformed depth can only come from the rotation).
    Frame 2 is one uniform colour, frame 3 is dark (values 0..12): contrast's mean and the clip at 0 are hit; the random frames hit the clip at 255."""
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    rgb[2] = np.array([200, 30, 90], np.uint8)
    rgb[3] = rs.randint(0, 13, (H, W, 3)).astype(np.uint8)
    depth = (0.5 + 9.5 * rs.rand(n, H, W)).astype(np.float32)
    return rgb, depth


def to_records(params, dtype):
    """list of parameter dicts -> NumPy records of `dtype` (dataloaders.nyu.AUG_DTYPE == fd_aug_params)."""
    rec = np.zeros(len(params), dtype)
    for r, p in zip(rec, params):
        for k in ("s", "angle", "brightness", "contrast", "saturation"):
            r[k] = p[k]
        r["flip"], r["order"] = int(p["flip"]), p["order"]
    return rec


def from_record(r):
    """one NumPy record (fd_aug_params) -> the parameter dict the two restatements take."""
    return dict(s=float(r["s"]), angle=float(r["angle"]), flip=bool(r["flip"]), brightness=float(r["brightness"]), contrast=float(r["contrast"]),
                saturation=float(r["saturation"]), order=tuple(int(v) for v in r["order"]))
