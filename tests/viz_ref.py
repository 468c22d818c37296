"""NumPy restatement of the reference's comparison rows (utils.py:37-74 colored_depthmap / merge_into_row / merge_into_row_with_gt and
deploy/data/visualize.py:22-31) as the bytes its save_image writes (`.astype('uint8')`), and the cases the CPU and the GPU tier share.

No matplotlib: the colour table is the fixture tests/golden/viridis_u8.npy ([256, 3] uint8 = uint8(255 * viridis(i)[:3]), tools/make_golden_viz.py).
The arithmetic is matplotlib's Colormap.__call__ on a float32 array: t = rel * 256 in float32, t == 256 -> 255, t < 0 -> entry 0, t >= 256 -> entry 255,
NaN -> (0, 0, 0), otherwise int(t).  A NaN is never cast to an integer here."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_table = None


def table():
    global _table
    if _table is None:
        _table = np.load(os.path.join(GOLD, "viridis_u8.npy"))
        assert _table.shape == (256, 3) and _table.dtype == np.uint8
    return _table


def colour(depth, d_min, d_max):
    """[h, w] float32, float32 bounds -> [h, w, 3] uint8."""
    depth, d_min, d_max = np.asarray(depth, np.float32), np.float32(d_min), np.float32(d_max)
    with np.errstate(all="ignore"):
        rel = (depth - d_min) / (d_max - d_min)          # float32: one subtraction, one division
        t = rel * np.float32(256.0)
    assert rel.dtype == np.float32 and t.dtype == np.float32
    bad = np.isnan(t)
    t = np.where(bad, np.float32(0.0), t)                # (a NaN is not cast)
    idx = np.clip(t, np.float32(0.0), np.float32(255.0)).astype(np.int64)      # under -> 0; t == 256 and over -> 255; [255, 256) truncates to 255
    out = table()[idx]
    out[bad] = 0
    return out


def colour_panel(x_chw):
    """[3, h, w] float32 in [0, 1] -> [h, w, 3] uint8: uint8(double(255.0f * x)), truncated (saturating outside the range, NaN -> 0)."""
    v = (np.float32(255.0) * np.asarray(x_chw, np.float32)).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.trunc(np.clip(v, 0.0, 255.0)).astype(np.uint8).transpose(1, 2, 0)


def frame_range(maps_f):
    """float32 minimum / maximum over all pixels of a frame's maps; NumPy's min / max propagate NaN."""
    with np.errstate(all="ignore"):
        stack = np.stack([np.asarray(m, np.float32) for m in maps_f])
        return stack.min(), stack.max()


def paint_rows(x, maps, value_range=None):
    """x [n, 3, h, w] float32 or None, maps: 1..3 arrays [n, 1, h, w] (or [n, h, w]) float32, value_range [n, 2] or None
    -> [n * h, panels * w, 3] uint8 = np.vstack of the reference's rows."""
    maps = [np.asarray(m, np.float32).reshape(m.shape[0], m.shape[-2], m.shape[-1]) for m in maps]
    n = maps[0].shape[0]
    rows = []
    for f in range(n):
        lo, hi = frame_range([m[f] for m in maps]) if value_range is None else (value_range[f][0], value_range[f][1])
        panels = ([colour_panel(x[f])] if x is not None else []) + [colour(m[f], lo, hi) for m in maps]
        rows.append(np.hstack(panels))
    return np.vstack(rows)


def sample():
    """The golden sample: x = float32(sample_rgb_u8) / 255 as [1, 3, 224, 224], the recorded target and the recorded prediction."""
    rgb = np.load(os.path.join(GOLD, "sample_rgb_u8.npy"))
    x = (rgb.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)[None]
    d = np.load(os.path.join(GOLD, "sample_depth.npy")).astype(np.float32).reshape(1, 1, 224, 224)
    p = np.load(os.path.join(GOLD, "sample_tvm_pred.npy")).astype(np.float32).reshape(1, 1, 224, 224)
    return np.ascontiguousarray(x), d, p


def _depths(g, n, h, w, zeros=0):
    d = (0.7 + 9.3 * g.random((n, 1, h, w), dtype=np.float32)).astype(np.float32)
    if zeros:
        flat = d.reshape(-1)
        flat[g.choice(flat.size, zeros, replace=False)] = 0.0
    return d


_cases = None


def cases():
    """name -> dict(x, maps, value_range, pitch_extra).  Built once, shared, never modified by a test."""
    global _cases
    if _cases is not None:
        return _cases
    g = np.random.default_rng(20261018)
    c = {}
    # A: odd sizes (byte path), a pitch 5 bytes larger than the row
    c["A"] = dict(x=g.random((3, 3, 5, 7), dtype=np.float32), maps=[_depths(g, 3, 5, 7), _depths(g, 3, 5, 7)], value_range=None, pitch_extra=5)
    # B: the dword path, three maps, depths in [0.7, 10] with some exact zeros
    c["B"] = dict(x=g.random((2, 3, 32, 36), dtype=np.float32), maps=[_depths(g, 2, 32, 36, 9), _depths(g, 2, 32, 36, 9), _depths(g, 2, 32, 36)],
                  value_range=None, pitch_extra=0)
    # C: one constant pixel, no colour panel: 0 / 0 -> black
    c["C"] = dict(x=None, maps=[np.full((1, 1, 1, 1), 2.5, np.float32)], value_range=None, pitch_extra=0)
    # D: one NaN in map1 of frame 1
    d0, d1 = _depths(g, 3, 8, 12), _depths(g, 3, 8, 12)
    d1[1, 0, 3, 5] = np.nan
    c["D"] = dict(x=g.random((3, 3, 8, 12), dtype=np.float32), maps=[d0, d1], value_range=None, pitch_extra=0)
    d1c = d1.copy()
    d1c[1, 0, 3, 5] = 4.0
    c["D_clean"] = dict(x=c["D"]["x"], maps=[d0, d1c], value_range=None, pitch_extra=0)
    # E: +Inf and -Inf in different frames, an explicit range inside the data (under, over, rel == 1 at d == d_max), the colour values that pin the truncation
    e0, e1 = _depths(g, 2, 8, 12), _depths(g, 2, 8, 12)
    e0[0, 0, 1, 2] = np.inf
    e1[1, 0, 6, 7] = -np.inf
    rng = np.array([[2.0, 7.5], [1.25, 9.0]], np.float32)
    for f in range(2):
        e0[f, 0, 0, 0] = rng[f, 1]                       # d == d_max: rel == 1, t == 256 -> 255
        e1[f, 0, 0, 1] = rng[f, 0]                       # d == d_min: entry 0
        e0[f, 0, 0, 2] = rng[f, 0] - np.float32(1.0)     # under
        e1[f, 0, 0, 3] = rng[f, 1] + np.float32(1.0)     # over
    xe = g.random((2, 3, 8, 12), dtype=np.float32)
    vals = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255.0), np.array([0.0, 1.0, 0.999999], np.float32)])
    xe.reshape(-1)[:vals.size] = vals                    # 259 of the 576 values
    assert (e0 < rng[:, 0].reshape(2, 1, 1, 1)).any() and (e1 > rng[:, 1].reshape(2, 1, 1, 1)).any()
    c["E"] = dict(x=xe, maps=[e0, e1], value_range=rng, pitch_extra=0)
    # F: a frame spans many workgroups in both launches
    c["F"] = dict(x=g.random((32, 3, 224, 224), dtype=np.float32), maps=[_depths(g, 32, 224, 224), _depths(g, 32, 224, 224)], value_range=None, pitch_extra=0)
    for v in c.values():
        for a in [v["x"]] + v["maps"] + [v["value_range"]]:
            if a is not None:
                a.setflags(write=False)
    _cases = c
    return c


_wants = {}


def want(name):
    """The expected canvas of a case (computed once)."""
    if name not in _wants:
        c = cases()[name] if name != "sample" else None
        if c is None:
            x, d, p = sample()
            w = paint_rows(x, [d, p])
        else:
            w = paint_rows(c["x"], c["maps"], c["value_range"])
        w.setflags(write=False)
        _wants[name] = w
    return _wants[name]


def png_decode(data):
    """An 8-bit RGB, non-interlaced PNG -> [h, w, 3] uint8, with zlib by hand (all five filter types)."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, shape = 8, b"", None
    while pos < len(data):
        ln, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + ln]
        assert struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])[0] == (zlib.crc32(kind + body) & 0xffffffff), kind
        if kind == b"IHDR":
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
            shape = (h, w)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + ln
    h, w = shape
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.uint8)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        up = out[y - 1].astype(np.int32) if y else np.zeros(3 * w, np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = line + up
        else:
            cur = np.zeros(3 * w, np.int32)
            for i in range(3 * w):
                a = cur[i - 3] if i >= 3 else 0
                b = up[i]
                cc = up[i - 3] if i >= 3 else 0
                if ft == 1:
                    pr = a
                elif ft == 3:
                    pr = (a + b) // 2
                else:
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pr = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                cur[i] = (line[i] + pr) & 255
        out[y] = cur & 255
    return out.reshape(h, w, 3)
