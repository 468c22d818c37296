"""Comparison rows on the device (C ABI fd_depth_rows): `colour frame | depth map ...` per frame as 8-bit RGB, the depth panels viridis-coloured over
the frame's joint range -- the bytes the reference's utils.merge_into_row / merge_into_row_with_gt / colored_depthmap give after save_image's
`.astype('uint8')` (include/fastdepth_hip.h states the arithmetic).  The canvas leaves the device as uint8, 3 bytes per pixel.

    canvas = viz.paint_rows(x, target, pred)                 # uint8 [n * h, 3 * w, 3] on the device
    viz.save_png(canvas, "comparison.png")                   # zlib + struct only

encode_png / save_png write 8-bit RGB PNG files with the standard library alone (no PIL)."""
import struct
import zlib

import numpy as np
import torch

from . import capi


def _as_maps(maps):
    out = []
    for m in maps:
        if m.dim() == 2:
            m = m[None]
        if m.dim() == 4:
            if m.shape[1] != 1:
                raise ValueError("a depth map is [n, 1, h, w], [n, h, w] or [h, w]; got %s" % (tuple(m.shape),))
            m = m[:, 0]
        if m.dim() != 3:
            raise ValueError("a depth map is [n, 1, h, w], [n, h, w] or [h, w]; got %s" % (tuple(m.shape),))
        out.append(m)
    return out


def paint_rows(x, *maps, value_range=None, out=None, _library=None):
    """x: [n, 3, h, w] (or [3, h, w]) float32 in [0, 1], or None for no colour panel; maps: one to three depth maps [n, 1, h, w], [n, h, w] or [h, w]
    float32, all on x's device; value_range: None (each frame's own minimum / maximum over its maps, NaN-propagating), a (d_min, d_max) pair for all
    frames, or an [n, 2] tensor / array.  Returns a uint8 tensor [n * h, panels * w, 3] on the same device, or paints into `out`: a uint8 view of that
    shape (or wider) whose pixels are contiguous (strides (pitch, 3, 1)); bytes of `out` beyond the panels are left as they are.  Nothing synchronises.
    `_library`: a loaded library to call instead of the product's (the CPU tier passes the emulator build with CPU tensors)."""
    if not 1 <= len(maps) <= 3:
        raise ValueError("one to three depth maps, got %d" % len(maps))
    maps = _as_maps(maps)
    n, h, w = maps[0].shape
    dev = maps[0].device
    if x is not None:
        if x.dim() == 3:
            x = x[None]
        if tuple(x.shape) != (n, 3, h, w):
            raise ValueError("the colour frames are [%d, 3, %d, %d] like the maps; got %s" % (n, h, w, tuple(x.shape)))
    tensors = ([x] if x is not None else []) + maps
    for t in tensors:
        if t.dtype != torch.float32 or t.device != dev or tuple(t.shape[-2:]) != (h, w) or t.shape[0] != n:
            raise ValueError("colour frames and depth maps are float32 tensors of one device and one [n, h, w]; got %s %s on %s" % (tuple(t.shape), t.dtype, t.device))
    if _library is None:
        if not maps[0].is_cuda:
            raise RuntimeError("paint_rows runs on the GPU (no CPU fallback); got tensors on %s" % dev)
        from .engine import lib
        L = lib()
    else:
        L = _library
    tensors = [t.contiguous() for t in tensors]
    xc = tensors[0] if x is not None else None
    mc = tensors[1:] if x is not None else tensors
    panels = len(tensors)
    if out is None:
        out = torch.empty((n * h, panels * w, 3), dtype=torch.uint8, device=dev)
    elif (out.dtype != torch.uint8 or out.device != dev or out.dim() != 3 or out.shape[0] != n * h or out.shape[1] < panels * w or out.shape[2] != 3
          or out.stride(2) != 1 or out.stride(1) != 3 or (n * h > 1 and out.stride(0) < panels * w * 3)):
        raise ValueError("out is a uint8 [%d, >= %d, 3] view on %s with contiguous pixels; got %s %s strides %s on %s"
                         % (n * h, panels * w, dev, tuple(out.shape), out.dtype, tuple(out.stride()), out.device))
    pitch = out.stride(0) if n * h > 1 else max(out.stride(0), panels * w * 3)
    rng = scratch = None
    if value_range is not None:
        rng = value_range if torch.is_tensor(value_range) else torch.from_numpy(np.array(value_range, np.float32))
        rng = rng.to(device=dev, dtype=torch.float32)
        if rng.dim() == 1:
            rng = rng[None].expand(n, 2)
        if tuple(rng.shape) != (n, 2):
            raise ValueError("value_range is (d_min, d_max) or [n, 2]; got %s" % (tuple(rng.shape),))
        rng = rng.contiguous()
    else:
        scratch = torch.empty(L.fd_depth_rows_scratch_bytes(n), dtype=torch.uint8, device=dev)

    def call(stream):
        ptr = [m.data_ptr() for m in mc] + [None] * (3 - len(mc))
        capi.check(L, L.fd_depth_rows(xc.data_ptr() if xc is not None else None, ptr[0], ptr[1], ptr[2], n, h, w, rng.data_ptr() if rng is not None else None,
                                      out.data_ptr(), pitch, scratch.data_ptr() if scratch is not None else None, stream), "fd_depth_rows")

    if maps[0].is_cuda:
        with torch.cuda.device(dev):
            call(torch.cuda.current_stream(dev).cuda_stream)
    else:
        call(None)
    return out


def encode_png(array):
    """[h, w, 3] uint8 (NumPy array or tensor on any device) -> the bytes of an 8-bit RGB PNG file (filter 0 on every line, one IDAT chunk)."""
    if torch.is_tensor(array):
        array = array.detach().cpu().numpy()
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("an image is a uint8 [h, w, 3] array; got %s %s" % (a.shape, a.dtype))
    h, w = a.shape[:2]
    lines = np.zeros((h, 1 + 3 * w), np.uint8)          # every line: filter type 0, then the pixels
    lines[:, 1:] = a.reshape(h, 3 * w)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(lines.tobytes(), 6))
            + chunk(b"IEND", b""))


def save_png(array, path):
    data = encode_png(array)
    with open(path, "wb") as f:
        f.write(data)
