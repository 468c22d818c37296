"""Drop-in for the reference's utils.py (its lines 12-83): parse_command, colored_depthmap, merge_into_row, merge_into_row_with_gt, add_row,
save_image -- the comparison image painted on the GPU (fastdepth_hip.viz.paint_rows, C ABI fd_depth_rows) and written without PIL.

One difference in type, none in the file that comes out: the reference's painters return the float64 image and its save_image casts it with
`.astype('uint8')`; here the painters return NumPy **uint8** arrays, and the contract is equality with what the reference's save_image writes.
add_row and save_image accept either form (a float image is cast as the reference casts it), so code written against the reference -- paint, add_row,
save_image -- runs unchanged.  The painters take torch tensors on the device or NumPy arrays (uploaded first); there is no CPU painter.  A NaN in ANY of
the maps of a frame blackens that frame's depth panels (the reference's min(np.min(a), np.min(b)) drops a NaN that is not in the first map)."""
import numpy as np
import torch

from fastdepth_hip import viz


def parse_command(argv=None):
    from evaluate import parse_command as parse
    return parse(argv)


def _device_tensor(a, _library):
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))
    a = a.detach().to(torch.float32)
    if _library is None and not a.is_cuda:
        a = a.cuda()
    return a


def _frame(a, _library, channels):
    """The reference squeezes its inputs: [1, c, h, w], [c, h, w] (or [1, 1, h, w], [1, h, w], [h, w] for a map) -> [1, c, h, w] / [1, h, w]."""
    a = _device_tensor(a, _library)
    h, w = a.shape[-2:]
    if a.numel() != channels * h * w:
        raise ValueError("expected ONE frame with %d channel(s), got a tensor of shape %s" % (channels, tuple(a.shape)))
    return a.reshape(1, 3, h, w) if channels == 3 else a.reshape(1, h, w)


def _paint(x, maps, value_range, _library):
    return viz.paint_rows(x, *maps, value_range=value_range, _library=_library).cpu().numpy()


def colored_depthmap(depth, d_min=None, d_max=None, _library=None):
    """[h, w] depth -> [h, w, 3] uint8, viridis over [d_min, d_max] (default: the map's own minimum / maximum).  Reference utils.py:37-43."""
    d = _frame(depth, _library, 1)
    if d_min is None and d_max is None:
        return _paint(None, [d], None, _library)
    lo = d.amin() if d_min is None else torch.as_tensor(np.float32(d_min), device=d.device)      # amin / amax propagate NaN, as np.min / np.max
    hi = d.amax() if d_max is None else torch.as_tensor(np.float32(d_max), device=d.device)
    return _paint(None, [d], torch.stack([lo.reshape(()), hi.reshape(())]).to(torch.float32), _library)


def merge_into_row(input, depth_target, depth_pred, _library=None):
    """`rgb | target | prediction` of one frame, [h, 3 w, 3] uint8.  Reference utils.py:46-57."""
    return _paint(_frame(input, _library, 3), [_frame(depth_target, _library, 1), _frame(depth_pred, _library, 1)], None, _library)


def merge_into_row_with_gt(input, depth_input, depth_target, depth_pred, _library=None):
    """`rgb | sparse input | target | prediction`, [h, 4 w, 3] uint8.  Reference utils.py:60-74."""
    return _paint(_frame(input, _library, 3), [_frame(m, _library, 1) for m in (depth_input, depth_target, depth_pred)], None, _library)


def _image(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if a.dtype == np.uint8 else a.astype('uint8')


def add_row(img_merge, row):
    return np.vstack([_image(img_merge), _image(row)])


def save_image(img_merge, filename):
    """Writes an 8-bit RGB PNG (fastdepth_hip.viz.encode_png: zlib + struct).  Reference utils.py:81-83."""
    viz.save_png(_image(img_merge), filename)
